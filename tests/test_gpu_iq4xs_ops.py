"""GPU: the IQ4_XS kernels through the C-ABI (include/bamd.h bamd_op_*) against the genuine reference's stored outputs (tests/golden/iq4xs_kats.npz) and, at the
shapes the stored cases do not have, against the numpy restatement that tests/test_iq4xs_ref.py holds to those outputs (tests/iq4xs_ref.py).  Bit equality
throughout; every expectation is finite.  The edge blocks (scales at both ends, qs all 0x00 / 0xFF, d subnormal / largest / negative / zero, zero activation
blocks, activation blocks that hold every byte -127 .. 127) go through every launch form: they are stored cases."""
import os

import numpy as np
import pytest

import iq4xs_ref as xr
from bitcheck import ADD, EPS, SILU_MUL, STORE, assert_bits, normed, silu_mul
from booster_amd.gguf import random_iq4_xs_tensor, random_kquant_tensor
from conftest import GOLDEN
from test_iq4xs_ref import stored, stored_case  # noqa: F401  (stored: fixture)

pytestmark = pytest.mark.gpu
T = xr.IQ4_XS
Q5_K, Q6_K = 13, 14
PRO_NORM, PRO_PLAIN = 1, 0
GENERIC = 16                                                  # mode + 16: the generic kernels forced
MODES = (0, 1, 2, 1 + GENERIC, 2 + GENERIC)                   # the launcher's choice, one wave per row-group, split-K (where K / 256 has a split shape), and the last two on the generic kernels


def ref(po, t, W, rows, K, a):
    if t == T:
        return xr.mul_mat(po, W, rows, K, a)
    return po.mul_mat_q(t, W, rows, K, np.ascontiguousarray(a, np.float32), nthreads=8)[0]


# ---- the reference's own outputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_mul_mat_vec_kats(bamd, stored, mode):
    """every stored case — K = 256, 768 (three super-blocks: ring depth 1), 4096, 14336, the edge blocks and the pairs case — in every launch mode"""
    for key, blocks, xs, digest, _ in xr.all_cases():
        dots, _, _ = stored_case(stored, key, digest)
        K = xs[0].size
        for i, x in enumerate(xs):
            assert_bits(bamd.op_mul_mat_vec(T, blocks, xr.ROWS, K, x, mode=mode), dots[i], "%s vector %d mode %d" % (key, i, mode))


def test_the_quantiser_never_writes_minus_128(bamd):
    """the premise under which the kernels' product sum is the plain signed dot (bamd_device.h): no Q8_K byte of any stored activation vector is -128"""
    for key, _, xs, _, _ in xr.all_cases():
        for i, x in enumerate(xs):
            q8 = bamd.op_quantize_q8_K(x)
            assert not (xr.ei.q8_fields(q8)[1] == -128).any(), "%s vector %d" % (key, i)


def test_mul_mat_vec_kats_residual_and_ragged_rows(bamd, stored):
    """the stored dots with a residual add, and the first 29 rows only (a ragged last row-group)"""
    rng = np.random.default_rng(5 + T)
    for key, blocks, xs, digest, _ in xr.all_cases():
        dots, _, _ = stored_case(stored, key, digest)
        K = xs[0].size
        rb = K // 256 * xr.BB
        res = rng.standard_normal(xr.ROWS).astype(np.float32)
        for mode in (0, 1, 2):
            assert_bits(bamd.op_mul_mat_vec(T, blocks, xr.ROWS, K, xs[1], residual=res, mode=mode), dots[1] + res, key + " + residual")
            assert_bits(bamd.op_mul_mat_vec(T, blocks[:29 * rb], 29, K, xs[2], mode=mode), dots[2][:29], key + " 29 rows")


def test_get_row_kats(bamd, stored):
    """embedding rows (dequantize_row_iq4_xs, two roundings): rows 0, 15, 31 of every random matrix, every row of the edge and pairs matrices"""
    for key, blocks, xs, digest, deq_rows in xr.all_cases():
        _, _, deq = stored_case(stored, key, digest)
        K = xs[0].size
        for i, r in enumerate(deq_rows):
            assert_bits(bamd.op_get_row(T, blocks, xr.ROWS, K, r), deq[i], "%s get_row %d" % (key, r))


def test_ffn_gate_up_kats(bamd, po, stored):
    """gate = rows 0-15, up = rows 16-31 of the stored matrices behind the RMSNorm prologue; the restatement is anchored to the stored dots first"""
    for key, blocks, xs, digest, _ in xr.all_cases():
        dots, _, _ = stored_case(stored, key, digest)
        K = xs[0].size
        rb = K // 256 * xr.BB
        assert_bits(xr.mul_mat(po, blocks, xr.ROWS, K, xs[1]), dots[1], key + ": restatement")
        w = np.ones(K, np.float32)
        y = xr.mul_mat(po, blocks, xr.ROWS, K, normed(po, xs[1], w))
        got = bamd.op_ffn_gate_up(T, blocks[:16 * rb], blocks[16 * rb:], 16, K, xs[1], norm_w=w, eps=EPS)
        assert_bits(got, silu_mul(po, y[:16], y[16:]), key + " gate/up")


@pytest.mark.parametrize("nt", [1, 2, 7, 33])
def test_mul_mat_batch_kats(bamd, stored, nt):
    """the integer-dot batched kernel: token rows cycle through the stored activation vectors (expectation = the stored dots); a residual at odd T"""
    rng = np.random.default_rng(nt + T)
    for key, blocks, xs, digest, _ in xr.all_cases():
        dots, _, _ = stored_case(stored, key, digest)
        K = xs[0].size
        pick = [i % len(xs) for i in range(nt)]
        X = np.stack([xs[i] for i in pick])
        res = rng.standard_normal((nt, xr.ROWS)).astype(np.float32) if nt % 2 else None
        got = bamd.op_mul_mat_batch(T, blocks, xr.ROWS, K, X, residual=res, impl=0)
        want = np.stack([dots[i] for i in pick])
        assert_bits(got, want if res is None else want + res, "%s T %d" % (key, nt))


# ---- every launch mode at the shapes of the issue, expectation from the restatement -------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 512, 768, 4096, 5120, 14336])
def test_mul_mat_vec_shapes(bamd, po, K):
    """ring depths 1 (K = 768), 2 (512), 4 (5120) and 8; split-K with 1, 2, 7 records per wave and the uneven split of 20 super-blocks (K = 5120); 8, 24 and a
    ragged 20 rows; plain and RMSNorm prologue, with and without residual"""
    rng = np.random.default_rng(1000 * T + K)
    W = random_iq4_xs_tensor(K, 24, rng)
    rb = K // 256 * xr.BB
    x = (rng.standard_normal(K) * 3).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    res = rng.standard_normal(24).astype(np.float32)
    plain, norm = xr.mul_mat(po, W, 24, K, x), xr.mul_mat(po, W, 24, K, normed(po, x, w))
    for rows in (8, 24, 20):
        for mode in MODES:
            what = "K %d rows %d mode %d" % (K, rows, mode)
            Wr = W[:rows * rb]
            assert_bits(bamd.op_mul_mat_vec(T, Wr, rows, K, x, mode=mode), plain[:rows], what)
            assert_bits(bamd.op_mul_mat_vec(T, Wr, rows, K, x, residual=res[:rows], mode=mode), plain[:rows] + res[:rows], what + " + residual")
            assert_bits(bamd.op_mul_mat_vec(T, Wr, rows, K, x, norm_w=w, eps=EPS, mode=mode), norm[:rows], what + " norm")
            assert_bits(bamd.op_mul_mat_vec(T, Wr, rows, K, x, norm_w=w, eps=EPS, residual=res[:rows], mode=mode), norm[:rows] + res[:rows], what + " norm + residual")


@pytest.mark.parametrize("K,rows,norm", [(4096, 4096, False), (14336, 4096, False), (4096, 2056, True)])
def test_wo_and_ffn_down_shapes(bamd, po, K, rows, norm):
    """the 8B launches wo and ffn_down (plain + residual over 4096 rows: two row-groups per workgroup, split-K with two and seven records per wave) and a ragged
    RMSNorm launch with more row-groups than workgroups"""
    rng = np.random.default_rng(31 + T + K + rows)
    W = random_iq4_xs_tensor(K, rows, rng)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32) if norm else None
    res = None if norm else rng.standard_normal(rows).astype(np.float32)
    want = xr.mul_mat(po, W, rows, K, x if w is None else normed(po, x, w))
    if res is not None:
        want = want + res
    for mode in (0, 1, 2):
        assert_bits(bamd.op_mul_mat_vec(T, W, rows, K, x, norm_w=w, eps=EPS, residual=res, mode=mode), want, "K %d rows %d mode %d" % (K, rows, mode))


@pytest.mark.parametrize("K,mode", [(4096, 0), (4096, GENERIC), (768, 0)])
def test_argmax(bamd, po, K, mode):
    """the lm_head launch with its greedy arg-max epilogue, the largest logit tied between rows of different workgroups: logits and the lowest tied row"""
    rows = 2056
    rng = np.random.default_rng(60 + T + K + mode)
    W = random_iq4_xs_tensor(K, rows, rng).reshape(rows, -1)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    a = normed(po, x, w)
    y0 = xr.mul_mat(po, W.reshape(-1), rows, K, a)
    tied = [8 * 100 + 5, 8 * 101 + 2, rows - 1]
    top, bottom = int(np.argmax(y0)), int(np.argmin(y0))
    best = W[top].copy()
    W[top] = W[bottom]
    W[tied] = best
    want = xr.mul_mat(po, W.reshape(-1), rows, K, a)
    assert np.flatnonzero(want == want.max()).tolist() == tied
    got, row = bamd.op_mul_mat_vec_argmax(T, W.reshape(-1), rows, K, x, norm_w=w, eps=EPS, mode=mode)
    assert_bits(got, want, "lm_head logits")
    assert row == tied[0]


@pytest.mark.parametrize("K,rows", [(512, 40), (4096, 14336), (2816, 40)])   # 14336 rows on 256 CUs: seven row-group pairs per workgroup
def test_ffn_gate_up_shapes(bamd, po, K, rows):
    rng = np.random.default_rng(5 * T + K)
    Wg = random_iq4_xs_tensor(K, rows, rng, amp=4.0)
    Wu = random_iq4_xs_tensor(K, rows, rng, amp=4.0)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    a = normed(po, x, w)
    want = silu_mul(po, xr.mul_mat(po, Wg, rows, K, a), xr.mul_mat(po, Wu, rows, K, a))
    assert_bits(bamd.op_ffn_gate_up(T, Wg, Wu, rows, K, x, norm_w=w, eps=EPS), want, "ffn gate/up K %d rows %d" % (K, rows))


# ---- the fused QKV launch: one Q8_K launch with mixed segments ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("types", [(T, T, Q5_K), (T, T, T)])
@pytest.mark.parametrize("E,rows", [(512, (512, 128, 128)), (4096, (4096, 1024, 1024)), (768, (72, 13, 24))])
def test_fused_qkv(bamd, po, types, E, rows):
    """the recipe's QKV — IQ4_XS attn_q / attn_k beside a Q5_K attn_v (n_gqa >= 4) — and the uniform one, behind one RMSNorm prologue in ONE launch, in every
    mode: the tiny and the 8B widths, and ragged segments at three super-blocks"""
    rng = np.random.default_rng([31, E] + list(types))
    Ws = [random_kquant_tensor(t, E, r, rng) for t, r in zip(types, rows)]
    x = (rng.standard_normal(E) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(E)).astype(np.float32)
    a = normed(po, x, w)
    want = np.concatenate([ref(po, t, W, r, E, a) for t, W, r in zip(types, Ws, rows)])
    for mode in MODES:
        got = bamd.op_fused_qkv([(t, W, r) for t, W, r in zip(types, Ws, rows)], E, x, w, eps=EPS, mode=mode)
        assert_bits(got, want, "fused QKV %r E %d mode %d" % (types, E, mode))


def test_fused_qkv_edge_blocks(bamd, po, stored):
    """the edge matrix as attn_q and attn_k beside a Q5_K attn_v, on the edge activation vectors (behind RMSNorm with unit weights)"""
    blocks, xs, digest, _, _ = xr.edge_case()
    rng = np.random.default_rng(77)
    K = xr.EDGE_K
    rb = K // 256 * xr.BB
    V = random_kquant_tensor(Q5_K, K, 16, rng)
    w = np.ones(K, np.float32)
    segs = [(T, blocks[:16 * rb], 16), (T, blocks[16 * rb:], 16), (Q5_K, V, 16)]
    for x in xs:
        a = normed(po, x, w)
        want = np.concatenate([ref(po, t, W, r, K, a) for t, W, r in segs])
        for mode in MODES:
            assert_bits(bamd.op_fused_qkv(segs, K, x, w, eps=EPS, mode=mode), want, "edge QKV mode %d" % mode)


# ---- launch selection -----------------------------------------------------------------------------------------------------------------------------------
def test_launches_land_on_own_instances_or_the_generic_kernels(bamd):
    """a launch with an IQ4_XS segment takes an instance of ITS type or the generic kernels (which dispatch per segment), never another type's instance: the
    mangled name of whatever is chosen holds Li23E (the type as a template argument), or it is matvec_kernel / matvec_split_kernel"""
    shapes = [([(T, 4096)], 4096, PRO_PLAIN, ADD), ([(T, 4096)], 14336, PRO_PLAIN, ADD), ([(T, 6144)], 4096, PRO_NORM, STORE),
              ([(T, 5120), (Q5_K, 1024)], 4096, PRO_NORM, STORE), ([(T, 14336), (T, 14336)], 4096, PRO_NORM, SILU_MUL), ([(T, 28672), (T, 28672)], 8192, PRO_NORM, SILU_MUL),
              ([(T, 32000)], 4096, PRO_NORM, 3), ([(T, 24)], 768, PRO_PLAIN, STORE), ([(T, 8192)], 28672, PRO_PLAIN, ADD), ([(T, 1024)], 8192, PRO_PLAIN, ADD)]
    for segs, K, pro, epi in shapes:
        for mode in (0, 1, 2):
            if epi in (SILU_MUL, 3) and mode == 2:
                continue
            tr = bamd.trace_matvec(segs, K, pro, epi, mode)
            assert tr is not None, (segs, K, mode)
            k = tr["kernel"]
            generic = "13matvec_kernelIL" in k or "19matvec_split_kernelIL" in k
            assert generic or "Li23E" in k, "%r K %d mode %d went to %s" % (segs, K, mode, k)
    wo = bamd.trace_attn_wo(32, 8, 128, 512, 512, T, 4096, 4096)
    assert wo is not None and "attn_wo_kernel" in wo["kernel"] and "Li23E" in wo["kernel"]
    assert bamd.trace_matvec([(T, 4096), (20, 1024)], 4096, PRO_NORM, STORE) is None          # beside an IQ4_NL segment (Q8_0 activations): no kernel, refused on the host


def test_matrix_core_path_refuses_the_type(bamd, stored):
    """no matrix-core prompt kernel for IQ4_XS: impl 2 is an error in words, never wrong numbers; any other impl is the integer-dot kernel"""
    blocks, xs, digest = xr.rand_case(768)
    dots, _, _ = stored_case(stored, "iq4_xs_K768", digest)
    with pytest.raises(bamd.BamdError, match="MFMA path: unsupported type/shape"):
        bamd.op_mul_mat_batch(T, blocks, xr.ROWS, 768, np.stack(xs), impl=2)
    assert_bits(bamd.op_mul_mat_batch(T, blocks, xr.ROWS, 768, np.stack(xs), impl=1), dots, "impl 1")
    assert bamd.prefill_mfma_runs(T) == 0


# ---- prompt evaluation: the three epilogues of the segment form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,nt", [(256, 1), (4096, 2), (768, 7), (1536, 33), (14336, 7)])
def test_mul_mat_batch_epilogues(bamd, po, K, nt):
    """T tokens at once == the single-token launches of every token, and both == the restatement: STORE over IQ4_XS | IQ4_XS | Q5_K into one [T][ldo] matrix,
    ADD over one ragged matrix, SILU_MUL over a gate / up pair; ring depth 4 (K = 4096, 14336), 2 (1536) and 1 (256, 768)"""
    rng = np.random.default_rng(99 * T + K + nt)
    rows = [64, 16, 16]
    types = [T, T, Q5_K]
    Ws = [random_kquant_tensor(t, K, r, rng) for t, r in zip(types, rows)]
    X = (rng.standard_normal((nt, K)) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    A = [normed(po, X[i], w) for i in range(nt)]
    segs = [(t, W, r) for t, W, r in zip(types, Ws, rows)]
    ldo = sum(rows) + 8
    got = bamd.op_mul_mat_batch_seg(segs, K, X, ldo, epi=STORE, norm_w=w, eps=EPS, fill=-7.0)
    want = np.full((nt, ldo), -7.0, np.float32)
    for i in range(nt):
        want[i, :sum(rows)] = np.concatenate([ref(po, t, W, r, K, A[i]) for t, W, r in segs])
    assert_bits(got, want, "STORE q | k | v K %d T %d" % (K, nt))
    rb = K // 256 * xr.BB
    res = rng.standard_normal((nt, 13)).astype(np.float32)
    got = bamd.op_mul_mat_batch_seg([(T, Ws[0][:13 * rb], 13)], K, X, 13, epi=ADD, residual=res)
    assert_bits(got, np.stack([xr.mul_mat(po, Ws[0][:13 * rb], 13, K, X[i]) + res[i] for i in range(nt)]), "ADD K %d T %d" % (K, nt))
    got = bamd.op_mul_mat_batch_seg([(T, Ws[0][:16 * rb], 16), (T, Ws[1], 16)], K, X, 16, epi=SILU_MUL, norm_w=w, eps=EPS)
    want = np.stack([silu_mul(po, xr.mul_mat(po, Ws[0][:16 * rb], 16, K, A[i]), xr.mul_mat(po, Ws[1], 16, K, A[i])) for i in range(nt)])
    assert_bits(got, want, "SILU_MUL K %d T %d" % (K, nt))
    single = np.stack([bamd.op_ffn_gate_up(T, Ws[0][:16 * rb], Ws[1], 16, K, X[i], norm_w=w, eps=EPS) for i in range(nt)])
    assert_bits(got, single, "SILU_MUL vs the single-token launch")


# ---- attention and wo in one launch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hkv,hd,pos,rows", [(32, 8, 128, 37, "4096"), (32, 8, 128, 446, "ragged"), (64, 8, 64, 0, "extra_max"), (16, 2, 256, 255, "extra0")])
def test_attention_wo(bamd, po, H, Hkv, hd, pos, rows):
    """the wo role of the co-launched attention + wo kernel with an IQ4_XS wo at K = 4096, through tests/test_gpu_colaunch.py's run_case (attention role,
    granules, caches, x2) at its head layouts, positions and row kinds; the expectation of the wo rows comes from the restatement"""
    import test_gpu_colaunch as tc
    tc.run_case(bamd, po, T, H, Hkv, hd, 512, pos, rows, lds_ld=512, serial=3, step=pos + 1, il=T, gran_kind="ff" if pos else None,
                ref=lambda po_, t_, W, rows_, x: xr.mul_mat(po_, W, rows_, tc.K, x))


def test_attention_wo_edge_blocks(bamd, po):
    """the same launch with a wo made of the edge blocks (every edge kind in every record position of the 16 records of a row)"""
    import test_gpu_colaunch as tc
    rng = np.random.default_rng(4096 + T)
    W, _ = xr.edge_blocks(tc.K, 4096, rng)
    tc.run_case(bamd, po, T, 32, 8, 128, 512, 100, 4096, lds_ld=512, serial=2, step=101, il=1, W=W, what="edge wo",
                ref=lambda po_, t_, W_, rows_, x: xr.mul_mat(po_, W_, rows_, tc.K, x))


# ---- the sequential-order fallback of the RMSNorm f64 sum, at the kernel sites an IQ4_XS launch adds --------------------------------------------------------
@pytest.fixture(scope="module")
def okats():
    return np.load(os.path.join(GOLDEN, "f64_order_kats.npz"))


def firing(okats, name):
    """a constructed vector on which the guard fires whatever the summation tree (tests/test_gpu_f64_guard.py: firing_vector, with its CPU-side proof)"""
    from test_gpu_f64_guard import firing_vector
    return firing_vector(okats, name)


@pytest.mark.parametrize("name,layout,mode", [
    ("K4096", ((T, 5120), (Q5_K, 1024)), 0), ("K4096", ((T, 6144),), 0),                 # the launcher's choice for the recipe's and the uniform QKV
    ("K4096", ((T, 5120), (Q5_K, 1024)), 1 + GENERIC), ("K4096", ((T, 5120), (Q5_K, 1024)), 2 + GENERIC),
    ("K768", ((T, 40),), 1), ("K256", ((T, 64),), 1), ("K256", ((T, 64),), 2 + GENERIC), ("K3072", ((T, 3072), (T, 1024), (Q5_K, 1024)), 0),
])
def test_f64_guard_fallback_qkv(bamd, po, okats, name, layout, mode):
    from test_gpu_f64_guard import normed as normed_eps
    x, eps, K = firing(okats, name)
    rng = np.random.default_rng([K] + [v for t, r in layout for v in (t, r)])
    segs = [(t, random_kquant_tensor(t, K, r, rng, amp=4.0), r) for t, r in layout]
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    act = normed_eps(po, x, w, eps)
    want = np.concatenate([ref(po, t, W, r, K, act) for t, W, r in segs])
    for i in range(3):
        assert_bits(bamd.op_fused_qkv(segs, K, x, w, eps=eps, mode=mode), want, "guard %s %r mode %d call %d" % (name, layout, mode, i))


@pytest.mark.parametrize("name,rows", [("K4096", 14336), ("K768", 40)])
def test_f64_guard_fallback_gate_up(bamd, po, okats, name, rows):
    """gate/up with seven row-group pairs per workgroup (its IQ4_XS instance) and the generic kernel with the SiLU epilogue"""
    from test_gpu_f64_guard import normed as normed_eps
    x, eps, K = firing(okats, name)
    rng = np.random.default_rng([5, T, K, rows])
    Wg = random_iq4_xs_tensor(K, rows, rng, amp=4.0)
    Wu = random_iq4_xs_tensor(K, rows, rng, amp=4.0)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    act = normed_eps(po, x, w, eps)
    want = silu_mul(po, xr.mul_mat(po, Wg, rows, K, act), xr.mul_mat(po, Wu, rows, K, act))
    for i in range(3):
        assert_bits(bamd.op_ffn_gate_up(T, Wg, Wu, rows, K, x, norm_w=w, eps=eps), want, "guard gate/up %s rows %d call %d" % (name, rows, i))
