"""GPU: the matrix-core prompt mat-mul for IQ4_NL weights (matmul_mfma_b32_kernel<IQ4_NL, EPI>, booster_amd/csrc/bamd_prefill2_b32.hip, behind set_prefill_nl / BAMD_PREFILL_NL=1; default off).
Every expectation is the genuine reference's stored output (tests/golden/iq4nl_kats.npz, tests/golden/*iq4nl*.bgld) or the numpy restatement that
tests/test_iq4nl_ref.py holds to those (tests/iq4nl_ref.py); bit equality throughout, every expectation finite.  The switches are set through their setters and
restored afterwards to what the environment set; the launch counters (prefill_mfma_runs) tell the matrix-core kernel from the integer-dot kernel, which gives
the same bits.

Tile edges of the kernel: a workgroup is 64 rows x 16 tokens, a wave 16 rows x ONE token tile of 16 (wave and workgroup token tile coincide), a record group 8
rows."""
import numpy as np
import pytest

import iq4nl_ref as nl
import legacy_ref as lg
from bitcheck import ADD, EPS, FILL, SILU_MUL, STORE, assert_bits, normed, silu_mul
from booster_amd.gguf import random_iq4_nl_tensor, random_q0_tensor
from mfma_harness import layer_types, no_tables_with_the_switches_off, prefill_switches, prompt_step, runs, two_stages_on_the_matrix_cores
from refmodel import IQ4NL, load_fixture, model_for
from test_iq4nl_ref import stored, stored_case  # noqa: F401  (stored: fixture)

pytestmark = pytest.mark.gpu
NL = nl.IQ4_NL
Q4_0, Q8_0, Q5_K, Q6_K = lg.Q4_0, lg.Q8_0, 13, 14
COUNTED = [NL, Q4_0, lg.Q5_0, Q8_0, Q5_K, Q6_K]


def ref_batch(W, rows, K, A):
    return np.stack([nl.mul_mat(W, rows, K, a) for a in A])


def test_switch_is_off_by_default_and_refuses(bamd):
    """off: impl 2 declines the type as before and counts nothing — also with the Q8_0 family's switch on; on: it runs and counts.  (The first refusal is asked
    for before any setter call: under BAMD_PREFILL_NL=1 in the environment this test fails, by design.)"""
    blocks, xs, _ = nl.rand_case(256)
    before = runs(bamd, COUNTED)
    with pytest.raises(bamd.BamdError, match="MFMA path: unsupported type/shape"):
        bamd.op_mul_mat_batch(NL, blocks, nl.ROWS, 256, np.stack(xs), impl=2)
    with prefill_switches(bamd, nl=False, q0=True):
        with pytest.raises(bamd.BamdError, match="MFMA path: unsupported type/shape"):
            bamd.op_mul_mat_batch(NL, blocks, nl.ROWS, 256, np.stack(xs), impl=2)
    assert runs(bamd, COUNTED) == before
    with prefill_switches(bamd, nl=True, q0=False):
        bamd.op_mul_mat_batch(NL, blocks, nl.ROWS, 256, np.stack(xs), impl=2)
    after = runs(bamd, COUNTED)
    assert after[NL] == before[NL] + 1 and all(after[u] == before[u] for u in after if u != NL)


# ---- the reference's own outputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 7, 64])
def test_mul_mat_batch_kats(bamd, stored, T):
    """every stored case — K = 256, 512, 4096, 11008 and the edge matrix (d negative, zero, subnormal, large; all nibbles 0 / 15) — on the matrix-core kernel.
    K = 4096 is the case a one-accumulator chain fails (tests/test_iq4nl_ref.py, tests/test_iq4nl_mfma_math.py)"""
    rng = np.random.default_rng(T + NL)
    with prefill_switches(bamd, nl=True, q0=False):
        for key, blocks, xs, digest, _ in nl.all_cases():
            dots, _, _ = stored_case(stored, key, digest)
            K = xs[0].size
            pick = [i % len(xs) for i in range(T)]
            X = np.stack([xs[i] for i in pick])
            want = np.stack([dots[i] for i in pick])
            res = rng.standard_normal((T, nl.ROWS)).astype(np.float32)
            for r in (None, res):
                before = bamd.prefill_mfma_runs(NL)
                got = bamd.op_mul_mat_batch(NL, blocks, nl.ROWS, K, X, residual=r, impl=2)
                assert bamd.prefill_mfma_runs(NL) == before + 1
                assert_bits(got, want if r is None else want + r, "%s T %d residual %d" % (key, T, r is not None))
            if T == 7:                                # the first 29 rows only: a ragged last row-group, and rows of 29 floats (unaligned stores)
                rb = K // 32 * nl.BB
                got = bamd.op_mul_mat_batch(NL, blocks[:29 * rb], 29, K, X, residual=res[:, :29], impl=2)
                assert_bits(got, want[:, :29] + res[:, :29], "%s T %d, 29 rows" % (key, T))


# ---- shapes, expectation from the restatement ------------------------------------------------------------------------------------------------------
SHAPE_ROWS, SHAPE_T = 72, 65
_shape_ref = {}


def shape_ref(po, K, norm):
    """one matrix of 72 rows and 65 token rows per K, and W . Q8_0(x_t) of all of them with and without the RMSNorm prologue: the smaller shapes are the first
    rows and the first tokens of these"""
    if K not in _shape_ref:
        rng = np.random.default_rng(1013 * NL + K)
        W = random_iq4_nl_tensor(K, SHAPE_ROWS, rng)
        X = (rng.standard_normal((SHAPE_T, K)) * 3).astype(np.float32)
        w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        res = rng.standard_normal((SHAPE_T, SHAPE_ROWS)).astype(np.float32)
        _shape_ref[K] = dict(W=W, X=X, w=w, res=res)
    c = _shape_ref[K]
    if norm not in c:
        A = c["X"] if not norm else np.stack([normed(po, x, c["w"]) for x in c["X"]])
        c[norm] = ref_batch(c["W"], SHAPE_ROWS, K, A)
    return c, c[norm]


@pytest.mark.parametrize("K", [256, 512, 768])                  # one record (the prologue's stage only), two, an odd count
@pytest.mark.parametrize("rows", [8, 24, 72])                   # less than a wave's 16 rows, an odd row-group count, a partial second 64-row workgroup
@pytest.mark.parametrize("T", [1, 15, 16, 17, 32, 33, 65])      # both sides of the 16-token tile (wave = workgroup), two and four full tiles, a fifth with one token
def test_mul_mat_batch_shapes(bamd, po, K, rows, T):
    rb = K // 32 * nl.BB
    with prefill_switches(bamd, nl=True, q0=False):
        for norm in (False, True):
            c, want = shape_ref(po, K, norm)
            for with_res in (False, True):
                res = np.ascontiguousarray(c["res"][:T, :rows]) if with_res else None
                got = bamd.op_mul_mat_batch(NL, c["W"][:rows * rb], rows, K, c["X"][:T], norm_w=c["w"] if norm else None, eps=EPS, residual=res, impl=2)
                assert_bits(got, want[:T, :rows] + res if with_res else want[:T, :rows], "K %d rows %d T %d norm %d residual %d" % (K, rows, T, norm, with_res))


@pytest.mark.parametrize("rows", [16, 64])                      # exactly a wave's rows, exactly a workgroup's (the shapes above straddle both)
def test_mul_mat_batch_row_tile_edges(bamd, po, rows):
    K, T = 512, 33
    rb = K // 32 * nl.BB
    c, want = shape_ref(po, K, False)
    with prefill_switches(bamd, nl=True, q0=False):
        assert_bits(bamd.op_mul_mat_batch(NL, c["W"][:rows * rb], rows, K, c["X"][:T], impl=2), want[:T, :rows], "rows %d" % rows)


def test_mul_mat_batch_43_records(bamd, po):
    """K = 11008, the 43 records of Llama-2's ffn_down"""
    K, rows, T = 11008, 8, 3
    rng = np.random.default_rng(43 + NL)
    W = random_iq4_nl_tensor(K, rows, rng)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    res = rng.standard_normal((T, rows)).astype(np.float32)
    with prefill_switches(bamd, nl=True, q0=False):
        assert_bits(bamd.op_mul_mat_batch(NL, W, rows, K, X, impl=2), ref_batch(W, rows, K, X), "K 11008 plain")
        A = np.stack([normed(po, x, w) for x in X])
        assert_bits(bamd.op_mul_mat_batch(NL, W, rows, K, X, norm_w=w, eps=EPS, residual=res, impl=2), ref_batch(W, rows, K, A) + res, "K 11008 norm + residual")


def test_matrix_core_kernel_equals_integer_dot_kernel(bamd):
    K, rows, T = 4096, 256, 65
    rng = np.random.default_rng(4096 + NL)
    W = random_iq4_nl_tensor(K, rows, rng)
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    with prefill_switches(bamd, nl=True, q0=False):
        before = bamd.prefill_mfma_runs(NL)
        a = bamd.op_mul_mat_batch(NL, W, rows, K, X, norm_w=w, eps=EPS, impl=2)
        assert bamd.prefill_mfma_runs(NL) == before + 1
        b = bamd.op_mul_mat_batch(NL, W, rows, K, X, norm_w=w, eps=EPS, impl=1)
        assert bamd.prefill_mfma_runs(NL) == before + 1
    assert np.isfinite(b).all() and np.abs(b).max() > 0
    assert_bits(a, b, "impl 2 vs impl 1")


# ---- routing, as the engine issues the launches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [8, 9])                         # rows of a token 16-byte aligned, and not
def test_seg_two_iq4_nl_into_one_matrix(bamd, po, pad):
    """IQ4_NL | IQ4_NL (the q | k of the recipe's first launch group) into one [T][ldo]: one launch per segment, the fill behind the rows untouched"""
    K, T, rows = 512, 17, [256, 72]
    rng = np.random.default_rng(818 + pad)
    Ws = [random_iq4_nl_tensor(K, r, rng) for r in rows]
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    A = np.stack([normed(po, x, w) for x in X])
    ldo = sum(rows) + pad
    want = np.concatenate([ref_batch(W, r, K, A) for W, r in zip(Ws, rows)], axis=1)
    with prefill_switches(bamd, nl=True, q0=False):
        before = runs(bamd, COUNTED)
        got = bamd.op_mul_mat_batch_seg([(NL, W, r) for W, r in zip(Ws, rows)], K, X, ldo, epi=STORE, norm_w=w, eps=EPS, impl=2, fill=FILL)
        after = runs(bamd, COUNTED)
    assert after[NL] == before[NL] + 2 and all(after[u] == before[u] for u in after if u != NL)
    assert_bits(got[:, :sum(rows)], want, "q | k")
    assert (got[:, sum(rows):] == FILL).all(), "wrote behind the rows"


def test_seg_iq4_nl_beside_q8_0_with_only_this_switch(bamd, po):
    """IQ4_NL | IQ4_NL | Q8_0 in one call (one activation form), only BAMD_PREFILL_NL on: the IQ4_NL segments on the matrix cores, the Q8_0 one on the
    integer-dot kernel, all into one matrix"""
    K, T, rows = 512, 33, [64, 24, 16]
    rng = np.random.default_rng(819)
    Ws = [random_iq4_nl_tensor(K, rows[0], rng), random_iq4_nl_tensor(K, rows[1], rng), random_q0_tensor(Q8_0, K, rows[2], rng)]
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    want = np.concatenate([ref_batch(Ws[0], rows[0], K, X), ref_batch(Ws[1], rows[1], K, X), np.stack([lg.mul_mat(Q8_0, Ws[2], rows[2], K, x) for x in X])], axis=1)
    with prefill_switches(bamd, nl=True, q0=False):
        before = runs(bamd, COUNTED)
        got = bamd.op_mul_mat_batch_seg([(NL, Ws[0], rows[0]), (NL, Ws[1], rows[1]), (Q8_0, Ws[2], rows[2])], K, X, sum(rows) + 4, epi=STORE, impl=2, fill=FILL)
        after = runs(bamd, COUNTED)
    assert after[NL] == before[NL] + 2 and all(after[u] == before[u] for u in after if u != NL)
    assert_bits(got[:, :sum(rows)], want, "q | k | v")
    assert (got[:, sum(rows):] == FILL).all(), "wrote behind the rows"


@pytest.mark.parametrize("T", [7, 65])
def test_seg_silu_mul_pair(bamd, po, T):
    """gate, then up with h = silu(gate) * up as its in-place epilogue (res == out): two launches of the type, nothing written behind the rows"""
    K, rows = 512, 768
    rng = np.random.default_rng([51, NL, T])
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    Wg, Wu = random_iq4_nl_tensor(K, rows, rng, 4.0), random_iq4_nl_tensor(K, rows, rng, 4.0)
    A = np.stack([normed(po, x, w) for x in X])
    g, u = ref_batch(Wg, rows, K, A), ref_batch(Wu, rows, K, A)
    want = silu_mul(po, g.reshape(-1), u.reshape(-1)).reshape(T, rows)
    with prefill_switches(bamd, nl=True, q0=False):
        before = bamd.prefill_mfma_runs(NL)
        got = bamd.op_mul_mat_batch_seg([(NL, Wg, rows), (NL, Wu, rows)], K, X, rows + 64, epi=SILU_MUL, norm_w=w, eps=EPS, impl=2, fill=FILL)
        assert bamd.prefill_mfma_runs(NL) == before + 2
    assert_bits(got[:, :rows], want, "silu(gate) * up T %d" % T)
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"


@pytest.mark.parametrize("ldo", [832, 835])           # rows of a token 16-byte aligned, and not
def test_seg_add_with_wide_rows(bamd, po, ldo):
    """residual add with ldo > rows: output and residual share the stride, the columns behind the rows stay untouched"""
    K, rows, T = 512, 760, 65
    rng = np.random.default_rng([61, NL])
    X = (rng.standard_normal((T, K)) * 3).astype(np.float32)
    W = random_iq4_nl_tensor(K, rows, rng)
    res = rng.standard_normal((T, ldo)).astype(np.float32)
    want = ref_batch(W, rows, K, X) + res[:, :rows]
    with prefill_switches(bamd, nl=True, q0=False):
        before = bamd.prefill_mfma_runs(NL)
        got = bamd.op_mul_mat_batch_seg([(NL, W, rows)], K, X, ldo, epi=ADD, residual=res, impl=2, fill=FILL)
        assert bamd.prefill_mfma_runs(NL) == before + 1
    assert_bits(got[:, :rows], want, "add")
    assert (got[:, rows:] == FILL).all(), "wrote behind the rows"


# ---- whole models against the genuine reference's llama_decode ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["tiny_iq4nl", "tiny_iq4nl_mha", "tiny_iq4nl_imatrix_tied", "8bw_iq4nl"])
def test_whole_model_prompt_on_the_matrix_cores(bamd, cfg, monkeypatch, capfd):
    """the prompt step only: tables built (IQ4_NL plus K-quant matrices need this switch alone), no load-time complaint, the counters of the file's layer types
    move — on tiny_iq4nl the Q5_K one too: each launch group of the two-form QKV reaches its own matrix-core kernel — and the logits are the reference's"""
    fx = load_fixture(IQ4NL, cfg)
    path = model_for(IQ4NL, cfg, fx)
    low = layer_types(path, COUNTED)
    assert NL in low and low <= {NL, Q5_K, Q6_K}
    if cfg == "tiny_iq4nl":
        assert Q5_K in low
    monkeypatch.setenv("BAMD_PREFILL_VERBOSE", "1")
    err, aux, before, after = prompt_step(bamd, path, capfd, COUNTED, dict(nl=True, q0=False), fam=IQ4NL, cfg=cfg, fx=fx)
    assert "prompts run without the matrix-core kernels" not in err, err
    assert aux > 0
    for t in low:
        assert after[t] > before[t], "no matrix-core launch of type %d" % t
    no_tables_with_the_switches_off(bamd, path, "nl", "q0")


def test_prompt_through_two_stages_on_the_matrix_cores(bamd):
    """tiny_iq4nl through two layer-split stages (bamd_stage_prefill): the stage path takes the same routing"""
    two_stages_on_the_matrix_cores(bamd, IQ4NL, "tiny_iq4nl", COUNTED, (NL, Q5_K), dict(nl=True, q0=False))


def test_a_q4_0_matrix_beside_iq4_nl_needs_its_own_switch(bamd, tmp_path, monkeypatch, capfd):
    """a synthetic file whose ffn_down matrices are Q4_0 and whose other layer matrices are IQ4_NL.  Only BAMD_PREFILL_NL on: no tables, the reason names the
    missing switch, nothing on the matrix cores.  Both on: tables, both counters move"""
    from booster_amd import gguf
    path = str(tmp_path / "nl_q4_0.gguf")
    fn = lambda n, il: gguf.Q4_0 if n == "ffn_down" else gguf.Q6_K if n == "output" else gguf.IQ4_NL
    gguf.write_synthetic_llama(path, E=512, H=8, Hkv=8, L=2, F=768, V=64, type_fn=fn, embd_type=gguf.IQ4_NL, seed=5)
    monkeypatch.setenv("BAMD_PREFILL_VERBOSE", "1")
    err, aux, before, after = prompt_step(bamd, path, capfd, COUNTED, dict(nl=True, q0=False), n_prompt=19, n_ctx=64)
    assert aux == 0
    assert "prompts run without the matrix-core kernels" in err and "BAMD_PREFILL_Q0 is off" in err and "all-or-nothing per model" in err and "integer-dot kernel" in err, err
    assert after == before, "a launch on the matrix cores without side tables"
    err, aux, before, after = prompt_step(bamd, path, capfd, COUNTED, dict(nl=True, q0=True), n_prompt=19, n_ctx=64)
    assert "prompts run without the matrix-core kernels" not in err, err
    assert aux > 0 and after[NL] > before[NL] and after[Q4_0] > before[Q4_0]
