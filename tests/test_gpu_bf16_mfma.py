"""GPU: the matrix-core prompt mat-mul for BF16 weights (booster_amd/csrc/bamd_prefill2_bf16.hip, behind set_prefill_bf16 / BAMD_PREFILL_BF16=1; default off).
Every expectation is the genuine reference's stored output (tests/golden/float_kats.npz, the bf16_*_dots keys; tests/golden/float_*_bf16.bgld) or the numpy
restatement that tests/test_float_ref.py holds to those (tests/float_ref.py: the two-rounding chain); bit equality throughout, every expectation finite.  The
switch is set through the setter and restored afterwards; the launch counter prefill_mfma_runs(30) tells the matrix-core kernel from the VALU kernel, and
prefill_bf16_fallback_tiles() tells the kernel's two paths apart: the fma chain on the matrix cores where the exponent ranges prove every product exact, the
two-rounding step on the vector ALUs for a workgroup where they do not (the guard: tests/test_bf16_mfma_math.py).

Tile edges of the kernel (B_ROWS, B_TOK in bamd_prefill2_bf16.hip): a workgroup is 32 rows x 32 tokens, a wave ONE MFMA tile of 16 x 16, a record group 8 rows,
a record 256 of K = two MFMA steps.  So the row counts below are 8 (one row-group), 24 (a wave and a partial one), 40 (a partial second workgroup) and 72 (a
partial third); the token counts 1, 16, 17, 32, 33, 64, 65 are both sides of the MFMA tile = the wave's tokens, of the workgroup's 32 and of two workgroups."""
import contextlib
import os

import numpy as np
import pytest

import float_ref as fr
from bitcheck import ADD, EPS, FILL, SILU_MUL, STORE, assert_bits, normed, silu_mul
from booster_amd.gguf import random_float_tensor
from mfma_harness import layer_types, prompt_step, runs, two_stages_on_the_matrix_cores
from refmodel import FLOAT, load_fixture, model_for
from test_bf16_mfma_math import guard
from test_float_ref import stored  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
F32, F16, BF16 = fr.F32, fr.F16, fr.BF16
COUNTED = [F32, F16, BF16, 14]
WG_ROWS, WG_TOK = 32, 32                  # B_ROWS, B_TOK of booster_amd/csrc/bamd_prefill2_bf16.hip: the workgroup whose guard decides, and that the fallback counter counts
MESSAGE = "F32 / F16 / BF16 have no matrix-core kernel"


@contextlib.contextmanager
def bf16_switch(bamd, on=True):
    """the switch of this family through its setter; on exit it goes back to the process's default (mfma_harness.prefill_switches does not know it)"""
    bamd.set_prefill_bf16(on)
    try:
        yield
    finally:
        bamd.set_prefill_bf16(os.environ.get("BAMD_PREFILL_BF16", "")[:1] == "1")


def workgroups(rows, T):
    return -(-((rows + 7) // 8 * 8) // WG_ROWS) * -(-T // WG_TOK)


def ref_batch(W, rows, K, A):
    return np.stack([fr.mul_mat(BF16, W, rows, K, a) for a in A])


def is_safe(W, X):
    return all(guard(np.asarray(W, np.uint8).view(np.uint16), fr.bf16_bits(x)) for x in X)


def test_switch_is_off_by_default_and_refuses(bamd):
    """off, and with only flt on: impl 2 declines BF16 with the message it had before and counts nothing; on: it runs and counts type 30 alone; restored after"""
    W = random_float_tensor(BF16, 256, fr.ROWS, np.random.default_rng(2))
    X = np.random.default_rng(3).standard_normal((2, 256)).astype(np.float32)
    before = runs(bamd, COUNTED)

    def refused():
        with pytest.raises(bamd.BamdError, match=MESSAGE):
            bamd.op_mul_mat_batch(BF16, W, fr.ROWS, 256, X, impl=2)
        with pytest.raises(bamd.BamdError, match=MESSAGE):
            bamd.op_mul_mat_batch_seg([(BF16, W, fr.ROWS)], 256, X, fr.ROWS, epi=STORE, impl=2)
    with bf16_switch(bamd, False):
        refused()
        bamd.set_prefill_flt(True)
        try:
            refused()
        finally:
            bamd.set_prefill_flt(os.environ.get("BAMD_PREFILL_FLT", "")[:1] == "1")
        assert runs(bamd, COUNTED) == before
        with bf16_switch(bamd):
            got = bamd.op_mul_mat_batch(BF16, W, fr.ROWS, 256, X, impl=2)
            after = runs(bamd, COUNTED)
            with pytest.raises(bamd.BamdError, match="impl must be 0"):
                bamd.op_mul_mat_batch(BF16, W, fr.ROWS, 256, X, impl=1)
            assert runs(bamd, COUNTED) == after
        assert after[BF16] == before[BF16] + 1 and all(after[u] == before[u] for u in after if u != BF16)
        assert_bits(got, ref_batch(W, fr.ROWS, 256, X), "switch on")
        refused()                                     # restored


# ---- the reference's own outputs ---------------------------------------------------------------------------------------------------------------
def _kat(bamd, stored, key, raw, xs, digest, T, rng):
    """one stored case at T token rows cycling through its vectors, with and without residual (T = 7: also the first 29 rows only — a ragged last row-group and
    rows of 29 floats, unaligned stores); returns the launches made and the workgroups they had"""
    assert str(stored[key + "_inputs_sha256"]) == digest
    dots = stored[key + "_dots"]
    assert np.isfinite(dots).all()
    K = xs[0].size
    pick = [i % len(xs) for i in range(T)]
    X = np.stack([xs[i] for i in pick])
    want = np.stack([dots[i] for i in pick])
    res = rng.standard_normal((T, fr.ROWS)).astype(np.float32)
    launches = wgs = 0
    for r in (None, res):
        before = bamd.prefill_mfma_runs(BF16)
        got = bamd.op_mul_mat_batch(BF16, raw, fr.ROWS, K, X, residual=r, impl=2)
        assert bamd.prefill_mfma_runs(BF16) == before + 1
        assert_bits(got, want if r is None else want + r, "%s T %d residual %d" % (key, T, r is not None))
        launches += 1; wgs += workgroups(fr.ROWS, T)
    if T == 7:
        got = bamd.op_mul_mat_batch(BF16, raw[:29 * K * 2], 29, K, X, residual=res[:, :29], impl=2)
        assert_bits(got, want[:, :29] + res[:, :29], "%s T %d, 29 rows" % (key, T))
        launches += 1; wgs += workgroups(29, T)
    return launches, wgs


@pytest.mark.parametrize("T", [2, 7, 64])
def test_mul_mat_batch_kats(bamd, stored, T):
    """every stored bf16_K* case — K = 256, 512, 1024, 4096 at three scales — on the matrix cores: no workgroup falls back"""
    rng = np.random.default_rng(T + BF16)
    with bf16_switch(bamd):
        fb = bamd.prefill_bf16_fallback_tiles()
        for key, raw, xs, digest in fr.all_cases(BF16):
            if key != "bf16_edge":
                _kat(bamd, stored, key, raw, xs, digest, T, rng)
        assert bamd.prefill_bf16_fallback_tiles() == fb


@pytest.mark.parametrize("T", [2, 7, 64])
def test_mul_mat_batch_edge_kat_takes_the_two_rounding_path(bamd, stored, T):
    """the stored edge matrix x edge vectors (weight exponents down to -75, activation exponents down to -126: products below 2^-149, where the fma chain gives
    other bits than the stored answers for four of the six vectors): every workgroup launched falls back, and the answers are the reference's"""
    (key, raw, xs, digest), = [c for c in fr.all_cases(BF16) if c[0] == "bf16_edge"]
    with bf16_switch(bamd):
        fb = bamd.prefill_bf16_fallback_tiles()
        _, wgs = _kat(bamd, stored, key, raw, xs, digest, T, np.random.default_rng(T))
        assert bamd.prefill_bf16_fallback_tiles() == fb + wgs


def test_mixed_batch_falls_back_in_one_token_tile_only(bamd):
    """one unsafe edge vector among safe random tokens, 72 rows of edge weights (three row tiles), T = 70 (three token tiles): the token tile that holds the edge
    vector falls back in every row tile, the other two run on the matrix cores; all answers are the restatement's"""
    K, rows, T, at = fr.EDGE_K, 72, 70, 40
    rng = np.random.default_rng(7070)
    W, _ = fr.edge_weights(BF16, K, rows, rng)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    X[at] = fr.edge_case(BF16)[1][2]                     # the all-`tiny` vector
    assert is_safe(W, np.delete(X, at, axis=0)) and not is_safe(W, X[at:at + 1])
    assert workgroups(rows, T) == 9 and at // WG_TOK == 1
    want = ref_batch(W, rows, K, X)
    assert np.isfinite(want).all()
    with bf16_switch(bamd):
        fb = bamd.prefill_bf16_fallback_tiles()
        got = bamd.op_mul_mat_batch(BF16, W, rows, K, X, impl=2)
        assert bamd.prefill_bf16_fallback_tiles() == fb + 3      # the row tiles of one token tile
    assert_bits(got, want, "mixed batch")


# ---- shapes, expectation from the restatement ------------------------------------------------------------------------------------------------------
SHAPE_ROWS, SHAPE_T = 72, 65
_shape_ref = {}


def shape_ref(po, K, norm):
    """one matrix of 72 rows and 65 token rows per K, and W . x_t of all of them with and without the RMSNorm prologue: the smaller shapes are the first rows and
    the first tokens of these"""
    if K not in _shape_ref:
        rng = np.random.default_rng(1013 * (BF16 + 1) + K)
        W = random_float_tensor(BF16, K, SHAPE_ROWS, rng, amp=4.0)
        X = (rng.standard_normal((SHAPE_T, K)) * 3).astype(np.float32)
        w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        res = rng.standard_normal((SHAPE_T, SHAPE_ROWS)).astype(np.float32)
        for a in (W, X, w, res):
            a.setflags(write=False)
        _shape_ref[K] = dict(W=W, X=X, w=w, res=res)
    c = _shape_ref[K]
    if norm not in c:
        A = c["X"] if not norm else np.stack([normed(po, x, c["w"]) for x in c["X"]])
        assert is_safe(c["W"], A)
        c[norm] = ref_batch(c["W"], SHAPE_ROWS, K, A)
        assert np.isfinite(c[norm]).all()
        c[norm].setflags(write=False)
    return c, c[norm]


@pytest.mark.parametrize("K", [256, 512, 768])                  # one record (the prologue's stages only), two, an odd record count
@pytest.mark.parametrize("rows", [8, 24, 40, 72])
@pytest.mark.parametrize("T", [1, 16, 17, 32, 33, 64, 65])
def test_mul_mat_batch_shapes(bamd, po, K, rows, T):
    with bf16_switch(bamd):
        fb = bamd.prefill_bf16_fallback_tiles()
        for norm in (False, True):
            c, want = shape_ref(po, K, norm)
            for with_res in (False, True):
                res = np.ascontiguousarray(c["res"][:T, :rows]) if with_res else None
                before = bamd.prefill_mfma_runs(BF16)
                got = bamd.op_mul_mat_batch(BF16, c["W"][:rows * K * 2], rows, K, c["X"][:T], norm_w=c["w"] if norm else None, eps=EPS, residual=res, impl=2)
                assert bamd.prefill_mfma_runs(BF16) == before + 1
                assert_bits(got, want[:T, :rows] + res if with_res else want[:T, :rows], "K %d rows %d T %d norm %d residual %d" % (K, rows, T, norm, with_res))
        assert bamd.prefill_bf16_fallback_tiles() == fb


def test_mul_mat_batch_long_chain(bamd, po):
    """K = 14336, the 8B ffn_down: 112 chained MFMAs per tile"""
    K, rows, T = 14336, 8, 3
    rng = np.random.default_rng(43 + BF16)
    W = random_float_tensor(BF16, K, rows, rng, amp=4.0)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    res = rng.standard_normal((T, rows)).astype(np.float32)
    with bf16_switch(bamd):
        fb = bamd.prefill_bf16_fallback_tiles()
        assert_bits(bamd.op_mul_mat_batch(BF16, W, rows, K, X, impl=2), ref_batch(W, rows, K, X), "K 14336 plain")
        A = np.stack([normed(po, x, w) for x in X])
        assert_bits(bamd.op_mul_mat_batch(BF16, W, rows, K, X, norm_w=w, eps=EPS, residual=res, impl=2), ref_batch(W, rows, K, A) + res, "K 14336 norm + residual")
        assert bamd.prefill_bf16_fallback_tiles() == fb


def test_matrix_core_kernel_equals_valu_kernel(bamd):
    """beside the reference expectations above, not instead of them"""
    K, rows, T = 4096, 256, 65
    rng = np.random.default_rng(4096 + BF16)
    W = random_float_tensor(BF16, K, rows, rng, amp=4.0)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    with bf16_switch(bamd):
        before, fb = bamd.prefill_mfma_runs(BF16), bamd.prefill_bf16_fallback_tiles()
        a = bamd.op_mul_mat_batch(BF16, W, rows, K, X, norm_w=w, eps=EPS, impl=2)
        assert bamd.prefill_mfma_runs(BF16) == before + 1 and bamd.prefill_bf16_fallback_tiles() == fb
        b = bamd.op_mul_mat_batch(BF16, W, rows, K, X, norm_w=w, eps=EPS, impl=0)
        assert bamd.prefill_mfma_runs(BF16) == before + 1
    assert np.isfinite(b).all() and np.abs(b).max() > 0
    assert_bits(a, b, "impl 2 vs impl 0")


# ---- routing, as the engine issues the launches -------------------------------------------------------------------------------------------------------
def test_seg_qkv_into_one_matrix(bamd, po):
    """BF16 | BF16 | BF16 (q | k | v) into one [T][ldo]: one launch per segment, the fill behind the rows untouched"""
    K, T, rows = 512, 17, [136, 64, 72]
    rng = np.random.default_rng(808)
    Ws = [random_float_tensor(BF16, K, r, rng, amp=4.0) for r in rows]
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    A = np.stack([normed(po, x, w) for x in X])
    ldo = sum(rows) + 9
    want = np.concatenate([ref_batch(W, r, K, A) for W, r in zip(Ws, rows)], axis=1)
    with bf16_switch(bamd):
        before, fb = runs(bamd, COUNTED), bamd.prefill_bf16_fallback_tiles()
        got = bamd.op_mul_mat_batch_seg([(BF16, W, r) for W, r in zip(Ws, rows)], K, X, ldo, epi=STORE, norm_w=w, eps=EPS, impl=2, fill=FILL)
        after = runs(bamd, COUNTED)
        assert bamd.prefill_bf16_fallback_tiles() == fb
    assert after[BF16] == before[BF16] + 3 and all(after[u] == before[u] for u in after if u != BF16)
    assert_bits(got[:, :sum(rows)], want, "q | k | v")
    assert (got[:, sum(rows):] == FILL).all(), "wrote behind the rows"


@pytest.mark.parametrize("T", [7, 65])
def test_seg_silu_mul_pair(bamd, po, T):
    """gate, then up with h = silu(gate) * up as its in-place epilogue (res == out): two launches, nothing written behind the rows"""
    K, rows = 512, 200
    rng = np.random.default_rng([50, BF16, T])
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    Wg, Wu = random_float_tensor(BF16, K, rows, rng, amp=2.0), random_float_tensor(BF16, K, rows, rng, amp=2.0)
    A = np.stack([normed(po, x, w) for x in X])
    g, u = ref_batch(Wg, rows, K, A), ref_batch(Wu, rows, K, A)
    want = silu_mul(po, g.reshape(-1), u.reshape(-1)).reshape(T, rows)
    with bf16_switch(bamd):
        before = bamd.prefill_mfma_runs(BF16)
        got = bamd.op_mul_mat_batch_seg([(BF16, Wg, rows), (BF16, Wu, rows)], K, X, rows + 64, epi=SILU_MUL, norm_w=w, eps=EPS, impl=2, fill=FILL)
        assert bamd.prefill_mfma_runs(BF16) == before + 2
    assert_bits(got[:, :rows], want, "silu(gate) * up T %d" % T)
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"


@pytest.mark.parametrize("ldo", [832, 835])           # rows of a token 16-byte aligned, and not
def test_seg_add_with_wide_rows(bamd, po, ldo):
    """residual add with ldo > rows: output and residual share the stride, the columns behind the rows stay untouched"""
    K, rows, T = 256, 760, 65
    rng = np.random.default_rng([60, BF16])
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    W = random_float_tensor(BF16, K, rows, rng, amp=4.0)
    res = rng.standard_normal((T, ldo)).astype(np.float32)
    want = ref_batch(W, rows, K, X) + res[:, :rows]
    with bf16_switch(bamd):
        before = bamd.prefill_mfma_runs(BF16)
        got = bamd.op_mul_mat_batch_seg([(BF16, W, rows)], K, X, ldo, epi=ADD, residual=res, impl=2, fill=FILL)
        assert bamd.prefill_mfma_runs(BF16) == before + 1
    assert_bits(got[:, :rows], want, "add")
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"


# ---- whole models against the genuine reference's llama_decode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["tiny_bf16", "8bw_bf16"])
def test_whole_model_prompt_on_the_matrix_cores(bamd, cfg, monkeypatch, capfd):
    """the prompt step only, with the switch on: the reference's logits, BF16 launches counted, no side table, no note about a missing kernel"""
    fx = load_fixture(FLOAT, cfg)
    path = model_for(FLOAT, cfg, fx)
    monkeypatch.setenv("BAMD_PREFILL_VERBOSE", "1")
    assert layer_types(path, [BF16]) == {BF16}
    with bf16_switch(bamd):
        err, aux, before, after = prompt_step(bamd, path, capfd, COUNTED, {}, fam=FLOAT, cfg=cfg, fx=fx)
    assert "no matrix-core kernel" not in err, err
    assert aux == 0
    assert after[BF16] > before[BF16]


def test_prompt_through_two_stages_on_the_matrix_cores(bamd):
    """tiny_bf16 through two layer-split stages (bamd_stage_prefill): the stage path takes the same routing"""
    with bf16_switch(bamd):
        two_stages_on_the_matrix_cores(bamd, FLOAT, "tiny_bf16", COUNTED, (BF16,), {})
