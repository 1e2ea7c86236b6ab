"""GPU: every kernel family against the CPU oracle at the value edges its bit-exactness depends on (inputs: tests/edge_inputs.py), raw bits
compared as in tests/test_gpu_ops.py.  Every test also asserts its own coverage, so that a later change to the generators cannot quietly stop
reaching the edge it pins:
  test_quantize_q8_K_edges         the Q8_K prologue: first-max rule (opposite signs in one lane / two lanes), iscale overflow, .5 ties, +-0 blocks
  test_rmsnorm_rows_edges          the RMSNorm prologue on zero, tiny (f32-subnormal squares) and huge (squares overflow: scale 0) rows, + residual
  test_mul_mat_vec_edges           every weight / activation kind through each decode mat-vec class, modes 0 / 1 / 2
  test_mul_mat_batch_worst_tile    the exact int64 |isum| of the worst 32-element product reaches its bound; odd |S| > 2048 (the S_h / S_l split)
  test_mul_mat_batch_edges         edge-mixed matrices, T across the 16- and 64-token tiles, the batched RMSNorm prologue
  test_ffn_gate_up_silu_branches   gate values in every v_expf branch of SiLU, seven- and fourteen-pair kernels
  test_get_row_edges               dequantisation of every weight kind
  test_attention_*                 softmax rows reaching past -133 (subnormal and zero probabilities), the KV store at f16 ties / subnormals / -0
  test_argmax_ties                 the greedy arg-max epilogue: a maximum tied across workgroups and within a wave, the lowest row wins
"""
import numpy as np
import pytest

import edge_inputs as E
from bitcheck import assert_bits
from booster_amd.gguf import random_kquant_tensor

pytestmark = pytest.mark.gpu
TYPES = [12, 13, 14]
EPS = 1e-5
NT = 8
FLT_MIN = 2.0 ** -126
LOG2E = 1.4426950408889634


def oracle_act(po, x, norm_w):
    return x if norm_w is None else (po.rms_norm(x, EPS) * norm_w).astype(np.float32)


def oracle_mv(po, t, W, rows, K, X, norm_w=None):
    """the oracle's W . Q8_K(a) for every activation row of X (a = the RMSNorm prologue's output when norm_w is given): [T][rows], finite"""
    A = np.stack([oracle_act(po, x, norm_w) for x in np.atleast_2d(X)])
    y = po.mul_mat_q(t, W, rows, K, A, nthreads=NT)
    assert np.isfinite(y).all(), "edge inputs must keep the expected outputs finite"
    return y


def expf_branch(x):
    """the branch of ggml_v_expf an argument takes: 0 main, 1 |n| > 126 (scaled by 2^-+125: inf, or subnormal / 0), 2 |n| > 192"""
    n = np.abs(np.rint(np.asarray(x, np.float64) * LOG2E))
    return np.where(n > 192, 2, np.where(n > 126, 1, 0))


# ---- Q8_K prologue ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [False, True])
def test_quantize_q8_K_edges(bamd, po, norm):
    """plain: every activation kind six times; norm: the same through the RMSNorm prologue (a power-of-two weight per block keeps constant
    blocks constant).  Byte for byte, the sign of d included"""
    K = 256 * 60
    rng = np.random.default_rng(2024 + norm)
    x, tags = E.edge_activations(K, rng, huge_max=1e18 if norm else 1e30)
    w = np.repeat(2.0 ** rng.integers(-3, 4, K // 256), 256).astype(np.float32) if norm else None
    want = po.quantize_q8_K(oracle_act(po, x, w))
    d, qs, _ = E.q8_fields(want)
    assert np.isfinite(d).all()
    blocks = x.reshape(-1, 256)
    if not norm:
        om = tags == "opposite_max"
        assert om.sum() == 6 and np.array_equal(np.sign(d[om]), -E.first_max_sign(x)[om])      # d = -max / 127 of the FIRST extremum
        lanes = [len({int(i) // 4 for i in np.flatnonzero(np.abs(b) == np.abs(b).max())}) for b in blocks[om]]
        assert 1 in lanes and 2 in lanes                                                         # the pair in one lane and in two lanes
        ov = tags == "overflow_iscale"
        with np.errstate(over="ignore"):
            assert np.isinf(np.float32(-127.0) / np.abs(blocks[ov]).max(axis=1)).all()
        assert (d[ov] == 0).all() and not qs[ov].any()
        ti = np.flatnonzero(tags == "ties")
        mx = blocks[ti, np.argmax(np.abs(blocks[ti]), axis=1)]
        v = (np.float32(-127.0) / mx)[:, None].astype(np.float32) * blocks[ti]
        assert np.count_nonzero(v - np.floor(v) == 0.5) == 255 * ti.size                         # every element but the maximum is a tie
        assert (qs[tags == "constant"] == -127).all()
    z = tags == "zero"
    assert (d[z] == 0).all() and not qs[z].any()
    assert E.odd_pair_sums_above_2048(want) >= 8 * int((tags == "near_constant").sum())
    got = bamd.op_quantize_q8_K(x, norm_w=w, eps=EPS)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("t", TYPES)
def test_rmsnorm_rows_edges(bamd, po, t):
    """the RMSNorm prologue + residual epilogue on rows that are zero (+-0), tiny (f32-subnormal squares: the f64 sum leaves the range where
    the tree order is trusted, bamd_device.h f32_rounding_safe), vanishing (squares underflow to 0) and huge (squares overflow to inf: the
    reference's scale is 1 / sqrt(inf) = 0)"""
    K, rows = 4096, 512
    rng = np.random.default_rng(31 + t)
    W, _ = E.edge_kquant_tensor(t, K, rows, rng)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    res = rng.standard_normal(rows).astype(np.float32)
    g = rng.standard_normal(K)
    cases = {"zero": np.where(rng.random(K) < 0.5, -0.0, 0.0).astype(np.float32), "tiny": (g * 1e-21).astype(np.float32),
             "vanishing": (g * 1e-30).astype(np.float32), "huge": (g * 1e17).astype(np.float32), "overflow": (g * 1e20).astype(np.float32)}
    with np.errstate(over="ignore", under="ignore"):
        sq = {k: (v * v).astype(np.float32) for k, v in cases.items()}
    assert not sq["zero"].any() and ((sq["tiny"] > 0) & (sq["tiny"] < FLT_MIN)).sum() > K // 2 and not sq["vanishing"].any()
    assert np.isfinite(sq["huge"]).all() and np.isinf(sq["overflow"]).any()
    assert not po.rms_norm(cases["overflow"], EPS).any()
    for name, x in cases.items():
        want = oracle_mv(po, t, W, rows, K, x, w)[0] + res
        for mode in (0, 1, 2):
            got = bamd.op_mul_mat_vec(t, W, rows, K, x, norm_w=w, eps=EPS, residual=res, mode=mode)
            assert_bits(got, want, "%s row, type %d mode %d" % (name, t, mode))


# ---- decode mat-vec ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K,rows,norm,resid", [
    (768, 40, False, True),            # small K, ragged rows
    (4096, 512, False, False),
    (14336, 64, False, True),
    (28672, 2056, False, False),       # the 70B ffn_down: split-K with compact term buffers
    (8192, 8192, False, True),         # the 70B wo: four row-groups per workgroup + residual
    (4096, 6144, True, False),         # the fused QKV launch: RMSNorm prologue, three row-groups per workgroup
])
def test_mul_mat_vec_edges(bamd, po, t, K, rows, norm, resid):
    rng = np.random.default_rng(100 * t + K + rows)
    n_vec = -(-len(E.ACT_KINDS) // (K // 256))
    W, wt, X, xt = E.edge_matvec_inputs(t, K, rows, rng, n_vec=n_vec, huge_max=1e18 if norm else 1e30)
    assert set(wt.ravel()) == set(E.WEIGHT_KINDS) and set(xt.ravel()) == set(E.ACT_KINDS)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32) if norm else None
    res = rng.standard_normal(rows).astype(np.float32) if resid else None
    want = oracle_mv(po, t, W, rows, K, X, w)
    if not norm:
        assert sum(E.odd_pair_sums_above_2048(po.quantize_q8_K(x)) for x in X) >= 8
    for i, x in enumerate(X):
        wi = want[i] if res is None else want[i] + res
        for mode in (0, 1, 2):
            got = bamd.op_mul_mat_vec(t, W, rows, K, x, norm_w=w, eps=EPS, residual=res, mode=mode)
            assert_bits(got, wi, "type %d K %d rows %d mode %d vector %d" % (t, K, rows, mode, i))


# ---- batched prefill mat-mul ---------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("impl", [0, 2])
def test_mul_mat_batch_worst_tile(bamd, po, t, impl):
    """the largest integer products: every weight block `max` (Q6_K: the first 16-row tile with every scale -128 and every quant 0 -> -32),
    constant activation rows (every quant -127) and near-constant ones (odd pair sums just below 4064); T = 17 crosses the 16-token tile"""
    K, rows, T = 2048, 64, 17
    nb = K // 256
    rng = np.random.default_rng(7 * t + impl)
    W, _ = E.edge_kquant_tensor(t, K, rows, rng, kind_of=np.full((rows, nb), "max", dtype=object))
    Wb = W.reshape(rows * nb, -1)
    if t == 14:
        Wb[:16 * nb, 0:192] = 0
        Wb[:16 * nb, 192:208] = 0x80
    kinds = ["constant", "near_constant"] * 4 + [None] * (T - 8)
    X = np.stack([E.edge_activations(K, rng, kind_of=[k] * nb)[0] if k else E.edge_activations(K, rng)[0] for k in kinds])
    q8c, q8n = po.quantize_q8_K(X[0]), po.quantize_q8_K(X[1])
    assert int(np.abs(E.isum32(t, W, q8c)).max()) == E.ISUM_BOUND[t] and E.ISUM_BOUND[t] < 2 ** 24
    assert int(np.abs(E.pair_sums(q8c)).max()) == 32 * 127
    assert E.odd_pair_sums_above_2048(q8n) == 8 * nb
    want = oracle_mv(po, t, W, rows, K, X)
    got = bamd.op_mul_mat_batch(t, W, rows, K, X, impl=impl)
    for i in range(T):
        assert_bits(got[i], want[i], "worst tile, type %d impl %d token %d" % (t, impl, i))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("impl", [0, 2])
@pytest.mark.parametrize("T,norm", [(17, False), (65, True)])
def test_mul_mat_batch_edges(bamd, po, t, impl, T, norm):
    """edge-mixed matrices and activation rows; T = 17 (+ residual) and 65 (+ the batched RMSNorm prologue) cross the 16- and 64-token tiles"""
    K, rows = 2048, 40
    rng = np.random.default_rng(1000 * t + 10 * T + impl)
    W, wt, X, xt = E.edge_matvec_inputs(t, K, rows, rng, n_vec=T, huge_max=1e18 if norm else 1e30)
    assert set(wt.ravel()) == set(E.WEIGHT_KINDS) and set(xt.ravel()) == set(E.ACT_KINDS)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32) if norm else None
    res = None if norm else rng.standard_normal((T, rows)).astype(np.float32)
    want = oracle_mv(po, t, W, rows, K, X, w)
    if res is not None:
        want = want + res
    got = bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=EPS, residual=res, impl=impl)
    for i in range(T):
        assert_bits(got[i], want[i], "type %d T %d impl %d token %d" % (t, T, impl, i))


# ---- gate / up + SiLU --------------------------------------------------------------------------------------
def _scale_rows(t, W, rows, K, f):
    """multiply d (and dmin) of every super-block of row r by f[r], rounded to f16"""
    b = W.reshape(rows, K // 256, -1).copy()
    for off in ((208,) if t == 14 else (0, 2)):
        d = b[:, :, off:off + 2].copy().view(np.float16).astype(np.float64)
        b[:, :, off:off + 2] = (d * f[:, None, None]).astype(np.float16).view(np.uint8)
    return b.reshape(-1)


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K,rows", [(4096, 14336), (8192, 28672)])   # on 256 CUs: matvec_gateup7_kernel / matvec_gateup14_kernel
def test_ffn_gate_up_silu_branches(bamd, po, t, K, rows):
    """d of each gate row scaled so that the gate values are log-uniform in +-[1e-3, 1e3], with 64 rows in each band of SiLU's exp(-g):
    g in (-133, -87.3) and g < -133 (the overflow branch: a huge value or inf), g in (87.3, 133) and g > 133 (subnormal or 0), g near 0"""
    rng = np.random.default_rng(5 * t + K)
    Wg = random_kquant_tensor(t, K, rows, rng, amp=4.0)
    Wu = random_kquant_tensor(t, K, rows, rng, amp=4.0)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    g0 = oracle_mv(po, t, Wg, rows, K, x, w)[0].astype(np.float64)
    target = np.where(rng.random(rows) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-3, 3, rows)
    band = rng.permutation(rows)[:320].reshape(5, 64)
    target[band[0]] = -rng.uniform(95, 125, 64)
    target[band[1]] = -rng.uniform(140, 900, 64)
    target[band[2]] = rng.uniform(95, 125, 64)
    target[band[3]] = rng.uniform(140, 900, 64)
    target[band[4]] = np.where(rng.random(64) < 0.5, -1.0, 1.0) * rng.uniform(1e-4, 1e-2, 64)
    f = np.where(np.abs(g0) > 1e-3, target / np.where(g0 == 0, 1.0, g0), 1.0)
    Wg = _scale_rows(t, Wg, rows, K, f)
    g = oracle_mv(po, t, Wg, rows, K, x, w)[0]
    u = oracle_mv(po, t, Wu, rows, K, x, w)[0]
    for lo, hi in ((-133.0, -88.0), (-np.inf, -134.0), (88.0, 133.0), (134.0, np.inf), (-1e-2, 1e-2)):
        assert np.count_nonzero((g > lo) & (g < hi)) >= 32, "too few gate values in (%g, %g)" % (lo, hi)
    br = expf_branch(-g)
    assert np.count_nonzero(br == 1) >= 64 and np.count_nonzero(br == 2) >= 64
    s = po.silu(g)
    assert np.count_nonzero((s == 0) & (g < 0)) >= 64                                            # g / (1 + inf)
    want = s * u
    assert np.isfinite(want).all()
    got = bamd.op_ffn_gate_up(t, Wg, Wu, rows, K, x, norm_w=w, eps=EPS)
    assert_bits(got, want, "gate/up, type %d K %d" % (t, K))


# ---- embedding rows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
def test_get_row_edges(bamd, po, t):
    K, rows = 7 * 256, 14
    rng = np.random.default_rng(40 + t)
    kind_of = np.array([[E.WEIGHT_KINDS[(r + b) % 7] for b in range(7)] for r in range(rows)], dtype=object)
    W, _ = E.edge_kquant_tensor(t, K, rows, rng, kind_of=kind_of)
    rb = K // 256 * E.BLOCK_BYTES[t]
    n_negzero = 0
    for row in range(rows):
        want = po.dequantize(t, W[row * rb:(row + 1) * rb], K)
        assert np.isfinite(want).all()
        n_negzero += int(np.count_nonzero((want == 0) & np.signbit(want)))
        assert_bits(bamd.op_get_row(t, W, rows, K, row), want, "get_row type %d row %d" % (t, row))
    assert n_negzero > 0


# ---- attention -----------------------------------------------------------------------------------------------
# head 0's scaled scores relative to its maximum: the maximum, subnormal probabilities (-87.3 .. -104), 0 through the |n| > 126 branch, |n| > 192
PLANTED = (0.0, -90.0, -95.0, -100.0, -110.0, -125.0, -150.0, -300.0)


def identity_rope(hd):
    """(cos, sin) = (1, 0): RoPE leaves q and k as they are, so the current token's k reaches the f16 store at its edges"""
    return np.tile(np.array([1.0, 0.0], np.float32), hd // 2)


def attention_inputs(rng, H, Hkv, hd, n_ctx, pos):
    """K-cache rows below pos get head-0 scores q_0 . k / sqrt(hd) = 40 + PLANTED; V of KV head 0 is zero but at the rows of subnormal
    probability (so those alone make head 0's output); the current token's k / v are f16 edge values, head 0's k ties of magnitude 4 .. 16
    signed against q_0 so that its probability is 0"""
    Ekv = Hkv * hd
    kc = (rng.standard_normal(n_ctx * Ekv) * 0.7).astype(np.float16).view(np.uint16).copy()
    vc = rng.standard_normal(Ekv * n_ctx).astype(np.float16).view(np.uint16).copy()
    q = (rng.standard_normal(H * hd) * 2).astype(np.float32)
    q0 = q[:hd].astype(np.float64)
    rows = np.sort(rng.choice(pos, len(PLANTED), replace=False))
    vt = vc.reshape(Ekv, n_ctx)
    vt[:hd, :] = 0
    for i, p in zip(rows, PLANTED):
        kc[i * Ekv:i * Ekv + hd] = (q0 * ((40.0 + p) * np.sqrt(hd) / (q0 @ q0))).astype(np.float16).view(np.uint16)
        if -104 < p < -87:
            vt[:hd, i] = (rng.standard_normal(hd) * 1000).astype(np.float16).view(np.uint16)
    k = E.f16_edge_values(Ekv, rng)
    k[:hd] = -np.sign(q[:hd]) * np.abs(E.f16_ties_of(hd, rng, 2, 4))
    v = E.f16_edge_values(Ekv, rng)
    assert E.f16_ties(k) >= hd and E.f16_ties(v) > 0
    assert ((np.abs(v) < 2.0 ** -14) & (v != 0)).any() and (np.signbit(v) & (v == 0)).any()
    return q, k, v, kc, vc


def check_attention(bamd, po, H, Hkv, hd, n_ctx, pos, prefill, long_path, seed):
    from test_gpu_ops import oracle_attention
    rng = np.random.default_rng(seed)
    q, k, v, kc, vc = attention_inputs(rng, H, Hkv, hd, n_ctx, pos)
    rope = identity_rope(hd)
    kc2, vc2 = kc.copy(), vc.copy()
    want, wprobs = oracle_attention(po, q, k, v, kc2, vc2, rope, H, Hkv, hd, n_ctx, pos, prefill)
    assert np.isfinite(want).all()
    p = wprobs[:pos + 1]
    assert np.count_nonzero((p > 0) & (p < FLT_MIN)) >= 2 and np.count_nonzero(p == 0) >= 3       # subnormal and vanished probabilities
    assert 0 < np.abs(want[:hd]).max() < 1e-30                                                    # head 0's output is theirs alone
    if long_path:
        got, gprobs = bamd.op_attention(q, k, v, kc, vc, rope, H, Hkv, hd, n_ctx, pos, prefill_mode=prefill, want_probs=True)
        assert_bits(gprobs[:wprobs.size], wprobs, "softmax pos %d" % pos)
    else:
        got = bamd.op_attention(q, k, v, kc, vc, rope, H, Hkv, hd, n_ctx, pos, prefill_mode=prefill)
    assert np.array_equal(kc, kc2) and np.array_equal(vc, vc2), "KV store differs at pos %d" % pos
    assert_bits(got, want, "attention out pos %d" % pos)


@pytest.mark.parametrize("H,Hkv,hd", [(4, 1, 128), (8, 8, 64), (6, 2, 64)])
@pytest.mark.parametrize("prefill", [False, True])
@pytest.mark.parametrize("long_path", [False, True])
def test_attention_edges(bamd, po, H, Hkv, hd, prefill, long_path):
    """the fused path and (long_path) the three-kernel path with its probabilities, at n_ctx 256"""
    for pos in (100, 255):
        check_attention(bamd, po, H, Hkv, hd, 256, pos, prefill, long_path, H * 1000 + hd + pos + 2 * prefill)


@pytest.mark.parametrize("prefill", [False, True])
def test_attention_edges_softmax_pv_pair(bamd, po, prefill):
    """gq 4 at n_ctx 20480: attn_softmax_kernel + attn_pv_kernel beyond the register-cached pass"""
    check_attention(bamd, po, 4, 1, 128, 20480, 20479, prefill, True, 99 + prefill)


@pytest.mark.parametrize("impl,H,Hkv,hd,n_ctx,pos0,T", [(1, 8, 2, 128, 256, 100, 17), (2, 8, 2, 128, 256, 100, 17),
                                                       (1, 6, 2, 64, 192, 60, 9), (2, 16, 2, 128, 512, 300, 37)])
def test_attention_batch_edges(bamd, po, impl, H, Hkv, hd, n_ctx, pos0, T):
    """batched prefill attention (impl 1: VALU, 2: matrix cores) with q scaled so that a row's scores spread over more than 140 (far below
    the f16 range of the scores), the micro-batch's k / v at f16 ties, subnormals and -0"""
    rng = np.random.default_rng(impl * 1000 + H + T)
    Ekv = Hkv * hd
    kc = (rng.standard_normal(n_ctx * Ekv) * 0.7).astype(np.float16).view(np.uint16).copy()
    vc = rng.standard_normal(Ekv * n_ctx).astype(np.float16).view(np.uint16).copy()
    q = (rng.standard_normal((T, H * hd)) * 70).astype(np.float32)
    k = E.f16_edge_values(T * Ekv, rng, lo=-14, hi=1).reshape(T, Ekv)
    v = E.f16_edge_values(T * Ekv, rng).reshape(T, Ekv)
    assert E.f16_ties(k) > 0 and E.f16_ties(v) > 0
    rope = np.tile(identity_rope(hd), (n_ctx, 1))
    kf = kc.view(np.float16).astype(np.float64).reshape(n_ctx, Ekv)[:pos0, :hd]
    x = kf @ q[0, :hd].astype(np.float64) / np.sqrt(hd)
    rel = x - x.max()
    assert rel.min() < -140 and np.abs(x).max() * np.sqrt(hd) < 6e4
    assert np.count_nonzero((rel < -88) & (rel > -104)) >= 1 and np.count_nonzero(expf_branch(rel) == 2) >= 1
    kw, vw = kc.copy(), vc.copy()
    want = po.attention(q, k, v, kw, vw, rope, H, Hkv, hd, n_ctx, pos0, True)
    assert np.isfinite(want).all()
    got = bamd.op_attention_batch(q, k, v, kc, vc, rope, H, Hkv, hd, n_ctx, pos0, impl=impl)
    assert np.array_equal(kc, kw) and np.array_equal(vc, vw), "KV store differs"
    assert_bits(got, want, "batched attention impl %d" % impl)


# ---- greedy arg-max epilogue ----------------------------------------------------------------------------------
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("K,mode", [(4096, 0), (4096, 16), (1024, 0)])   # matvec_fast_kernel; the generic matvec_kernel (mode bit 4; K = 1024)
def test_argmax_ties(bamd, po, t, K, mode):
    """the largest logit copied into four rows: the lowest in the last workgroup, two in one wave of workgroup 0, one in workgroup 44; the
    epilogue (argmax_key + atomicMax over workgroups) must pick the lowest row, as std::max_element does"""
    rows = 4096
    rng = np.random.default_rng(60 + t + K + mode)
    W = random_kquant_tensor(t, K, rows, rng).reshape(rows, -1)
    x = (rng.standard_normal(K) * 2).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)
    y0 = oracle_mv(po, t, W, rows, K, x, w)[0]
    grid = min(256, rows // 8)
    tied = [8 * (grid - 1) + 5, 8 * grid + 2, 8 * grid + 6, 8 * (grid + 44) + 1]
    top, bottom = int(np.argmax(y0)), int(np.argmin(y0))
    best = W[top].copy()
    W[top] = W[bottom]
    W[tied] = best
    want = oracle_mv(po, t, W, rows, K, x, w)[0]
    assert np.flatnonzero(want == want.max()).tolist() == tied
    assert len({(r // 8) % grid for r in tied}) == 3 and (tied[1] // 8) % grid < (tied[0] // 8) % grid
    got, row = bamd.op_mul_mat_vec_argmax(t, W.reshape(-1), rows, K, x, norm_w=w, eps=EPS, mode=mode)
    assert_bits(got, want, "lm_head logits")
    assert row == int(np.argmax(want)) == tied[0]
