"""GPU: the matrix-core prompt mat-mul for F32 / F16 weights (booster_amd/csrc/bamd_prefill2_flt.hip, behind set_prefill_flt / BAMD_PREFILL_FLT=1; default off).
Every expectation is the genuine reference's stored output (tests/golden/float_kats.npz, the *_sgemm1 keys; tests/golden/float_*.bgld) or the numpy restatement
that tests/test_float_ref.py holds to those (tests/float_ref.py); bit equality throughout, every expectation finite.  The switch is set through the setter and
restored afterwards; the launch counters (prefill_mfma_runs) tell the matrix-core kernel from the VALU kernel, which gives the same bits.  BF16 has no such kernel.

Tile edges of the kernel: a workgroup is 64 rows x 64 tokens, a wave 32 rows x 32 tokens (2 x 2 MFMA tiles of 16 x 16), a record group 8 rows, a stage 128 of K
(two per record).  So the row counts below are 8, 24 (inside one wave), 32 (exactly a wave), 40 (a wave and a partial one), 64 (exactly a workgroup) and 72 (a
partial second workgroup); the token counts 1, 16, 17, 32, 33, 64, 65 are both sides of the MFMA tile, of the wave and of the workgroup."""
import numpy as np
import pytest

import float_ref as fr
from bitcheck import ADD, EPS, FILL, SILU_MUL, STORE, assert_bits, normed, silu_mul
from booster_amd.gguf import random_float_tensor
from mfma_harness import layer_types, prefill_switches, prompt_step, runs, two_stages_on_the_matrix_cores
from refmodel import FLOAT, load_fixture, model_for
from test_float_ref import stored  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
F32, F16, BF16 = fr.F32, fr.F16, fr.BF16
TYPES = [F32, F16]
COUNTED = TYPES + [14]


def ref_batch(t, W, rows, K, A):
    return np.stack([fr.mul_mat(t, W, rows, K, a) for a in A])


@pytest.mark.parametrize("t", TYPES)
def test_switch_is_off_by_default_and_refuses(bamd, t):
    """off: impl 2 declines the types as before and counts nothing; on: it runs and counts exactly the type launched; BF16 declines either way"""
    W = random_float_tensor(t, 256, fr.ROWS, np.random.default_rng(1))
    Wb = random_float_tensor(BF16, 256, fr.ROWS, np.random.default_rng(2))
    X = np.random.default_rng(3).standard_normal((2, 256)).astype(np.float32)
    before = runs(bamd, COUNTED)
    with pytest.raises(bamd.BamdError, match="F32 / F16 / BF16 have no matrix-core kernel"):
        bamd.op_mul_mat_batch(t, W, fr.ROWS, 256, X, impl=2)
    with pytest.raises(bamd.BamdError, match="F32 / F16 / BF16 have no matrix-core kernel"):
        bamd.op_mul_mat_batch_seg([(t, W, fr.ROWS)], 256, X, fr.ROWS, epi=STORE, impl=2)
    assert runs(bamd, COUNTED) == before
    with prefill_switches(bamd, flt=True):
        got = bamd.op_mul_mat_batch(t, W, fr.ROWS, 256, X, impl=2)
        after = runs(bamd, COUNTED)
        for args in ((BF16, Wb, fr.ROWS, 256, X),):
            with pytest.raises(bamd.BamdError, match="F32 / F16 / BF16 have no matrix-core kernel"):
                bamd.op_mul_mat_batch(*args, impl=2)
            with pytest.raises(bamd.BamdError, match="F32 / F16 / BF16 have no matrix-core kernel"):
                bamd.op_mul_mat_batch_seg([(BF16, Wb, fr.ROWS)], 256, X, fr.ROWS, epi=STORE, impl=2)
        with pytest.raises(bamd.BamdError, match="impl must be 0"):
            bamd.op_mul_mat_batch(t, W, fr.ROWS, 256, X, impl=1)
        assert runs(bamd, COUNTED) == after
    assert after[t] == before[t] + 1 and all(after[u] == before[u] for u in after if u != t)
    assert_bits(got, ref_batch(t, W, fr.ROWS, 256, X), "type %d" % t)
    with pytest.raises(bamd.BamdError, match="F32 / F16 / BF16 have no matrix-core kernel"):      # restored
        bamd.op_mul_mat_batch(t, W, fr.ROWS, 256, X, impl=2)


# ---- the reference's own outputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("T", [2, 7, 64])
def test_mul_mat_batch_kats(bamd, stored, t, T):
    """every stored case — K = 256, 512, 1024, 4096 and the edge matrix x edge vectors (subnormal f16 weights, f32 subnormal activations, products and partial
    sums below 2^-126, cancellation to a subnormal) — on the matrix-core kernel; the token rows cycle through the case's vectors"""
    rng = np.random.default_rng(T + t)
    with prefill_switches(bamd, flt=True):
        for key, raw, xs, digest in fr.all_cases(t):
            assert str(stored[key + "_inputs_sha256"]) == digest
            dots = stored[key + "_sgemm1"]
            K = xs[0].size
            pick = [i % len(xs) for i in range(T)]
            X = np.stack([xs[i] for i in pick])
            want = np.stack([dots[i] for i in pick])
            res = rng.standard_normal((T, fr.ROWS)).astype(np.float32)
            for r in (None, res):
                before = bamd.prefill_mfma_runs(t)
                got = bamd.op_mul_mat_batch(t, raw, fr.ROWS, K, X, residual=r, impl=2)
                assert bamd.prefill_mfma_runs(t) == before + 1
                assert_bits(got, want if r is None else want + r, "%s T %d residual %d" % (key, T, r is not None))
            if T == 7:                                # the first 29 rows only: a ragged last row-group, and rows of 29 floats (unaligned stores)
                rb = K * fr.ESIZE[t]
                got = bamd.op_mul_mat_batch(t, raw[:29 * rb], 29, K, X, residual=res[:, :29], impl=2)
                assert_bits(got, want[:, :29] + res[:, :29], "%s T %d, 29 rows" % (key, T))


def test_edge_answers_are_subnormal_results(stored):
    """what the case above carries for the subnormal question: non-zero stored answers below 2^-126 for both types"""
    for t in TYPES:
        a = stored["%s_edge_sgemm1" % fr.NAME[t]]
        assert ((np.abs(a) < 2.0 ** -126) & (a != 0)).sum() >= 4


# ---- shapes, expectation from the restatement ------------------------------------------------------------------------------------------------------
SHAPE_ROWS, SHAPE_T = 72, 65
_shape_ref = {}


def shape_ref(po, t, K, norm):
    """one matrix of 72 rows and 65 token rows per (type, K), and W . x_t of all of them with and without the RMSNorm prologue: the smaller shapes are the first
    rows and the first tokens of these"""
    if (t, K) not in _shape_ref:
        rng = np.random.default_rng(1013 * (t + 1) + K)
        W = random_float_tensor(t, K, SHAPE_ROWS, rng, amp=4.0)
        X = (rng.standard_normal((SHAPE_T, K)) * 3).astype(np.float32)
        w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        res = rng.standard_normal((SHAPE_T, SHAPE_ROWS)).astype(np.float32)
        for a in (W, X, w, res):
            a.setflags(write=False)
        _shape_ref[(t, K)] = dict(W=W, X=X, w=w, res=res)
    c = _shape_ref[(t, K)]
    if norm not in c:
        A = c["X"] if not norm else np.stack([normed(po, x, c["w"]) for x in c["X"]])
        c[norm] = ref_batch(t, c["W"], SHAPE_ROWS, K, A)
        c[norm].setflags(write=False)
    return c, c[norm]


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K", [256, 512, 768])                  # two stages (the prologue's and one more), four, an odd record count
@pytest.mark.parametrize("rows", [8, 24, 72])                   # one row-group, an odd row-group count inside a wave, a partial second 64-row workgroup
@pytest.mark.parametrize("T", [1, 16, 17, 32, 33, 64, 65])      # both sides of the 16-token tile, of the wave's 32 tokens and of the workgroup's 64
def test_mul_mat_batch_shapes(bamd, po, t, K, rows, T):
    rb = K * fr.ESIZE[t]
    with prefill_switches(bamd, flt=True):
        for norm in (False, True):
            c, want = shape_ref(po, t, K, norm)
            for with_res in (False, True):
                res = np.ascontiguousarray(c["res"][:T, :rows]) if with_res else None
                got = bamd.op_mul_mat_batch(t, c["W"][:rows * rb], rows, K, c["X"][:T], norm_w=c["w"] if norm else None, eps=EPS, residual=res, impl=2)
                assert_bits(got, want[:T, :rows] + res if with_res else want[:T, :rows], "type %d K %d rows %d T %d norm %d residual %d" % (t, K, rows, T, norm, with_res))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("rows", [16, 32, 40, 64])              # an MFMA tile; exactly a wave's rows; a wave and a partial one; exactly a workgroup's
def test_mul_mat_batch_row_tile_edges(bamd, po, t, rows):
    K, T = 512, 33
    rb = K * fr.ESIZE[t]
    c, want = shape_ref(po, t, K, False)
    with prefill_switches(bamd, flt=True):
        before = bamd.prefill_mfma_runs(t)
        assert_bits(bamd.op_mul_mat_batch(t, c["W"][:rows * rb], rows, K, c["X"][:T], impl=2), want[:T, :rows], "type %d rows %d" % (t, rows))
        assert bamd.prefill_mfma_runs(t) == before + 1


@pytest.mark.parametrize("t", TYPES)
def test_mul_mat_batch_long_chain(bamd, po, t):
    """K = 14336, the 8B ffn_down: 448 chained MFMAs per tile"""
    K, rows, T = 14336, 8, 3
    rng = np.random.default_rng(43 + t)
    W = random_float_tensor(t, K, rows, rng, amp=4.0)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    res = rng.standard_normal((T, rows)).astype(np.float32)
    with prefill_switches(bamd, flt=True):
        assert_bits(bamd.op_mul_mat_batch(t, W, rows, K, X, impl=2), ref_batch(t, W, rows, K, X), "K 14336 plain")
        A = np.stack([normed(po, x, w) for x in X])
        assert_bits(bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=EPS, residual=res, impl=2), ref_batch(t, W, rows, K, A) + res, "K 14336 norm + residual")


@pytest.mark.parametrize("t", TYPES)
def test_matrix_core_kernel_equals_valu_kernel(bamd, t):
    """beside the reference expectations above, not instead of them"""
    K, rows, T = 4096, 256, 65
    rng = np.random.default_rng(4096 + t)
    W = random_float_tensor(t, K, rows, rng, amp=4.0)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    with prefill_switches(bamd, flt=True):
        before = bamd.prefill_mfma_runs(t)
        a = bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=EPS, impl=2)
        assert bamd.prefill_mfma_runs(t) == before + 1
        b = bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=EPS, impl=0)
        assert bamd.prefill_mfma_runs(t) == before + 1
    assert np.isfinite(b).all() and np.abs(b).max() > 0
    assert_bits(a, b, "impl 2 vs impl 0")


# ---- routing, as the engine issues the launches -------------------------------------------------------------------------------------------------------
def test_seg_f16_beside_f32_into_one_matrix(bamd, po):
    """F16 | F32 | F16 (q | k | v of a mixed file) into one [T][ldo]: one launch per segment, the fill behind the rows untouched"""
    K, T, rows = 512, 17, [136, 64, 72]
    rng = np.random.default_rng(808)
    types = [F16, F32, F16]
    Ws = [random_float_tensor(t, K, r, rng, amp=4.0) for t, r in zip(types, rows)]
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    A = np.stack([normed(po, x, w) for x in X])
    ldo = sum(rows) + 9
    want = np.concatenate([ref_batch(t, W, r, K, A) for t, W, r in zip(types, Ws, rows)], axis=1)
    with prefill_switches(bamd, flt=True):
        before = runs(bamd, COUNTED)
        got = bamd.op_mul_mat_batch_seg([(t, W, r) for t, W, r in zip(types, Ws, rows)], K, X, ldo, epi=STORE, norm_w=w, eps=EPS, impl=2, fill=FILL)
        after = runs(bamd, COUNTED)
    assert after[F16] == before[F16] + 2 and after[F32] == before[F32] + 1 and after[14] == before[14]
    assert_bits(got[:, :sum(rows)], want, "q | k | v")
    assert (got[:, sum(rows):] == FILL).all(), "wrote behind the rows"


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("T", [7, 65])
def test_seg_silu_mul_pair(bamd, po, t, T):
    """gate, then up with h = silu(gate) * up as its in-place epilogue (res == out): two launches of the type, nothing written behind the rows"""
    K, rows = 512, 200
    rng = np.random.default_rng([50, t, T])
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    Wg, Wu = random_float_tensor(t, K, rows, rng, amp=2.0), random_float_tensor(t, K, rows, rng, amp=2.0)
    A = np.stack([normed(po, x, w) for x in X])
    g, u = ref_batch(t, Wg, rows, K, A), ref_batch(t, Wu, rows, K, A)
    want = silu_mul(po, g.reshape(-1), u.reshape(-1)).reshape(T, rows)
    with prefill_switches(bamd, flt=True):
        before = bamd.prefill_mfma_runs(t)
        got = bamd.op_mul_mat_batch_seg([(t, Wg, rows), (t, Wu, rows)], K, X, rows + 64, epi=SILU_MUL, norm_w=w, eps=EPS, impl=2, fill=FILL)
        assert bamd.prefill_mfma_runs(t) == before + 2
    assert_bits(got[:, :rows], want, "silu(gate) * up type %d T %d" % (t, T))
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("ldo", [832, 835])           # rows of a token 16-byte aligned, and not
def test_seg_add_with_wide_rows(bamd, po, t, ldo):
    """residual add with ldo > rows: output and residual share the stride, the columns behind the rows stay untouched"""
    K, rows, T = 256, 760, 65
    rng = np.random.default_rng([60, t])
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    W = random_float_tensor(t, K, rows, rng, amp=4.0)
    res = rng.standard_normal((T, ldo)).astype(np.float32)
    want = ref_batch(t, W, rows, K, X) + res[:, :rows]
    with prefill_switches(bamd, flt=True):
        before = bamd.prefill_mfma_runs(t)
        got = bamd.op_mul_mat_batch_seg([(t, W, rows)], K, X, ldo, epi=ADD, residual=res, impl=2, fill=FILL)
        assert bamd.prefill_mfma_runs(t) == before + 1
    assert_bits(got[:, :rows], want, "add type %d" % t)
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"


# ---- whole models against the genuine reference's llama_decode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["tiny_f16", "tiny_f32", "8bw_f16", "8bw_f32"])
def test_whole_model_prompt_on_the_matrix_cores(bamd, cfg, monkeypatch, capfd):
    """the prompt step only, with the switch on: the reference's logits, launches of the file's layer types counted, no side table"""
    fx = load_fixture(FLOAT, cfg)
    path = model_for(FLOAT, cfg, fx)
    monkeypatch.setenv("BAMD_PREFILL_VERBOSE", "1")
    err, aux, before, after = prompt_step(bamd, path, capfd, COUNTED, dict(flt=True), fam=FLOAT, cfg=cfg, fx=fx)
    assert "prompts run without the matrix-core kernels" not in err, err
    assert aux == 0
    low = layer_types(path, TYPES)
    assert low, "the fixture holds no F32 / F16 layer matrix"
    for t in low:
        assert after[t] > before[t], "no matrix-core launch of type %d" % t


def test_whole_bf16_model_stays_on_the_valu_kernel(bamd, monkeypatch, capfd):
    """tiny_bf16 with the switch on: the same logits, no launch counted for F32 / F16, and the load-time note still names the missing kernel"""
    fx = load_fixture(FLOAT, "tiny_bf16")
    path = model_for(FLOAT, "tiny_bf16", fx)
    monkeypatch.setenv("BAMD_PREFILL_VERBOSE", "1")
    err, aux, before, after = prompt_step(bamd, path, capfd, COUNTED, dict(flt=True), fam=FLOAT, cfg="tiny_bf16", fx=fx)
    assert aux == 0
    assert "no matrix-core kernel" in err, err
    assert after == before


def test_prompt_through_two_stages_on_the_matrix_cores(bamd):
    """tiny_f16 through two layer-split stages (bamd_stage_prefill): the stage path takes the same routing"""
    two_stages_on_the_matrix_cores(bamd, FLOAT, "tiny_f16", COUNTED, (F16,), dict(flt=True))
