"""The reference's double-precision sums are SEQUENTIAL (RMSNorm sum of squares, ggml.c:11874-11879; softmax denominator, :2619-2671); the GPU
reduces them as a fixed tree.  Both round to f32 at once (mean, 1 / sum), so the order shows only when the sum sits next to a rounding
boundary of that f32.  Round 3 closed the hole: f32_rounding_safe (bamd_device.h) bounds the reordering error, and when it cannot rule a
difference out one lane redoes the sum in the reference's order.  Pinned here on a CONSTRUCTED worst case (tests/golden/f64_order_kat.npz,
tools/f64_order_search.py) on which the two orders do differ — the means by one f32 ulp, 13 bytes of the Q8_K activations with them — and on
the guard's logic restated in numpy (it must fire on every vector on which the orders differ)."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def kat():
    return np.load(os.path.join(GOLDEN, "f64_order_kat.npz"))


def test_orders_differ_on_the_constructed_vector(kat, po):
    import f64_order_search as fs
    t = fs.terms(kat["x"])
    m_seq, m_tree = fs.mean32(fs.sum_seq(t)), fs.mean32(fs.sum_tree(t))
    assert m_seq.view(np.uint32) == kat["mean_seq"].view(np.uint32) and m_tree.view(np.uint32) == kat["mean_tree"].view(np.uint32)
    assert abs(int(m_seq.view(np.uint32)) - int(m_tree.view(np.uint32))) == 1
    # the oracle follows the reference: sequential
    assert np.array_equal(po.quantize_q8_K(po.rms_norm(kat["x"], float(kat["eps"]))), kat["q8k_seq"])
    assert not np.array_equal(kat["q8k_seq"], kat["q8k_tree"])


def test_guard_fires_on_the_constructed_vector_and_gives_the_sequential_mean(kat):
    import f64_order_search as fs
    m, fired = fs.guarded_mean32(fs.terms(kat["x"]))
    assert fired and m.view(np.uint32) == kat["mean_seq"].view(np.uint32)


def test_guard_never_misses(kat):
    """property: whenever the two orders give different f32 means the guard has fired — on random vectors and on a walk of the constructed
    vector's last element across the rounding boundary (where the orders disagree on a whole interval of steps)"""
    import f64_order_search as fs
    rng = np.random.default_rng(11)
    fired = 0
    for _ in range(1500):
        x = (rng.standard_normal(fs.K) * np.exp(rng.standard_normal(fs.K) * 2.0)).astype(np.float32)
        t = fs.terms(x)
        m, f = fs.guarded_mean32(t)
        fired += f
        assert m.view(np.uint32) == fs.mean32(fs.sum_seq(t)).view(np.uint32)
    assert fired < 15                                                   # ~1e-5 .. 1e-4 of natural reductions: the slow path stays rare
    x = kat["x"].copy()
    v0 = x[-1]
    differ = 0
    for k in range(-300, 300):
        x[-1] = np.float32(v0 * np.float32(1.0 + k * 2.0 ** -9))
        t = fs.terms(x)
        m, f = fs.guarded_mean32(t)
        a, b = fs.mean32(fs.sum_seq(t)), fs.mean32(fs.sum_tree(t))
        differ += int(a.view(np.uint32) != b.view(np.uint32))
        assert m.view(np.uint32) == a.view(np.uint32)
    assert differ >= 1


def test_random_vectors_agree():
    import f64_order_search as fs
    assert fs.random_trials(2000, np.random.default_rng(5)) == 0


@pytest.mark.gpu
def test_gpu_equals_the_reference_on_the_constructed_vector(kat, bamd):
    """the worst case through the HIP path: the guard sends it down the sequential order, so the bytes are the reference's"""
    got = bamd.op_quantize_q8_K(kat["x"], norm_w=np.ones(kat["x"].size, np.float32), eps=float(kat["eps"]))
    assert np.array_equal(got, kat["q8k_seq"])
    assert not np.array_equal(got, kat["q8k_tree"])


# ---- the softmax denominator (ggml.c:2619-2671): a constructed row of 64 scores (tests/golden/f64_softmax_kat.npz, tools/f64_softmax_search.py)
#      whose reciprocal sits on an f32 rounding boundary — the sequential order and a tree order of the same eight partial sums round to
#      DIFFERENT f32 (one ulp apart), so every probability of the row depends on the order ----
@pytest.fixture(scope="module")
def skat():
    return np.load(os.path.join(GOLDEN, "f64_softmax_kat.npz"))


def _softmax_row_orders(po, scores):
    import f64_softmax_search as ss
    e = ss.expf_table(po, scores * np.float32(0.125))
    return e, ss.denominators(e)


def test_softmax_orders_differ_on_the_constructed_row(skat, po):
    import f64_softmax_search as ss
    e, den = _softmax_row_orders(po, skat["scores"])
    inv_seq, inv_tree = np.float32(1.0 / den["seq"]), np.float32(1.0 / den["tree"])
    assert inv_seq.view(np.uint32) == skat["inv_seq"].view(np.uint32) and inv_tree.view(np.uint32) == skat["inv_tree"].view(np.uint32)
    assert abs(int(inv_seq.view(np.uint32)) - int(inv_tree.view(np.uint32))) == 1
    # the oracle follows the reference: sequential
    p = po.soft_max(skat["scores"], None, np.float32(0.125))
    assert np.array_equal(p.view(np.uint32), (e * inv_seq).astype(np.float32).view(np.uint32))
    assert not np.array_equal(p.view(np.uint32), (e * inv_tree).astype(np.float32).view(np.uint32))
    # whatever order a kernel adds the eight partial sums in, its reciprocal lies inside the band in which f32_rounding_safe (bamd_device.h)
    # refuses the fast path: |low 29 bits - 2^28| <= 2 n + 8, n = n_kv / 8
    for t in den.values():
        assert int(ss.dist(np.array([1.0 / t]))[0]) <= ss.GUARD_ULPS


@pytest.mark.gpu
@pytest.mark.parametrize("prefill", [False, True])
@pytest.mark.parametrize("long_path", [False, True])
def test_gpu_attention_equals_the_reference_on_the_constructed_row(skat, bamd, po, prefill, long_path):
    """the row through the HIP attention (single-launch kernel and the scores | softmax + P.V path): q = e_0, K rows = score x e_0 (f16-exact),
    identity RoPE, head dimension 64 (scale 1/8): the kernel's scores ARE the constructed row, its guard must take the sequential order.
    (A build with -DBAMD_NO_F64_GUARD fails this test on the single-launch kernel — 44 of 64 outputs one ulp off — and the RMSNorm test above;
    the softmax + P.V kernel's own tree happens to agree with the sequential order on this row, its fallback runs all the same.)"""
    from bitcheck import assert_bits
    from test_gpu_ops import oracle_attention
    H = Hkv = 1; hd = 64; n_ctx = 64; pos = 63
    s = skat["scores"]
    rng = np.random.default_rng(99)
    kc = np.zeros(n_ctx * hd, np.float16); kc[0::hd] = s.astype(np.float16); kc[pos * hd] = 0    # the token's own row comes from k
    kc = kc.view(np.uint16).copy()
    vc = rng.standard_normal(hd * n_ctx).astype(np.float16).view(np.uint16).copy()
    q = np.zeros(hd, np.float32); q[0] = 1.0
    k = np.zeros(hd, np.float32); k[0] = s[pos]
    v = rng.standard_normal(hd).astype(np.float32)
    rope = np.tile(np.array([1.0, 0.0], np.float32), hd // 2)
    kc2, vc2 = kc.copy(), vc.copy()
    want, wprobs = oracle_attention(po, q, k, v, kc2, vc2, rope, H, Hkv, hd, n_ctx, pos, prefill)
    e, den = _softmax_row_orders(po, s)
    assert np.array_equal(wprobs.view(np.uint32), (e * np.float32(1.0 / den["seq"])).astype(np.float32).view(np.uint32))    # the scores are the row
    if long_path:
        got, gprobs = bamd.op_attention(q, k, v, kc, vc, rope, H, Hkv, hd, n_ctx, pos, prefill_mode=prefill, want_probs=True)
        assert_bits(gprobs[:wprobs.size], wprobs, "softmax of the constructed row")
    else:
        got = bamd.op_attention(q, k, v, kc, vc, rope, H, Hkv, hd, n_ctx, pos, prefill_mode=prefill)
    assert_bits(got, want, "attention out on the constructed row")


# ---- constructed inputs for any length (tests/golden/f64_order_kats.npz, f64_softmax_kats.npz; tests/golden/gen_f64_guard_kats.py): the SEQUENTIAL value
#      sits within 8 units of an f32 rounding boundary, so every order of the same n terms (within 2 n units of it) lies inside the guard's band 2 n + 8:
#      the sequential fallback runs whatever a kernel's tree is.  tests/test_gpu_f64_guard.py drives every fallback site with them ----
ORDER_NAMES = ["K256", "K768", "K3072", "K4096", "K4096b", "K8192"]
SOFTMAX_NAMES = ["v64_p64_hd64", "v96_p96_hd64", "v576_p576_hd64", "v4128_p4128_hd64", "v8224_p8224_hd64", "v64_p64_hd128", "v96_p96_hd128",
                 "v80_p96_hd128", "v576_p576_hd128", "v64_p64_hd256", "v96_p96_hd64_holes", "v448_p448_hd128"]


@pytest.fixture(scope="module")
def okats():
    return np.load(os.path.join(GOLDEN, "f64_order_kats.npz"))


@pytest.fixture(scope="module")
def skats():
    return np.load(os.path.join(GOLDEN, "f64_softmax_kats.npz"))


def test_fixtures_hold_every_length(okats, skats):
    assert {n[2:] for n in okats.files if n.startswith("x_")} == set(ORDER_NAMES)
    assert {n[2:] for n in skats.files if n.startswith("s_")} == set(SOFTMAX_NAMES)
    assert np.array_equal(okats["x_K4096"], np.load(os.path.join(GOLDEN, "f64_order_kat.npz"))["x"])       # the existing vector meets the margin: reused


@pytest.mark.parametrize("name", ORDER_NAMES)
def test_rmsnorm_vector_sits_on_a_boundary_in_every_order(okats, po, name):
    import f64_order_search as fs
    x = okats["x_" + name]
    K = int(name[1:].rstrip("b"))
    assert x.size == K and x.dtype == np.float32
    o = fs.sum_orders(fs.terms(x))
    m_seq = fs.mean64(o["seq"], K)
    assert np.float32(m_seq).view(np.uint32) == okats["mean_" + name].view(np.uint32)
    assert int(fs.dist_units(m_seq)) <= fs.NEAR_UNITS == 8
    assert len(o) >= 3 and all(fs.guard_fires(s, K) for s in o.values())          # the sequential order and three others of the same terms
    assert list(okats["differs_" + name]) == sorted(n for n, s in o.items() if np.float32(fs.mean64(s, K)).view(np.uint32) != okats["mean_" + name].view(np.uint32))   # the recorded orders that round elsewhere
    if K == fs.K:
        assert fs.guarded_mean32(fs.terms(x))[1]                                  # ... and ActPro::finish's own tree at eight waves
    # the oracle's RMSNorm is the sequential mean
    scale = np.float32(1.0) / np.sqrt(np.float32(okats["mean_" + name] + okats["eps"]), dtype=np.float32)
    assert np.array_equal(po.rms_norm(x, float(okats["eps"])).view(np.uint32), (x * scale).astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("name", SOFTMAX_NAMES)
def test_softmax_row_sits_on_a_boundary_in_every_order(skats, po, name):
    import f64_softmax_search as ss
    s, scale = skats["s_" + name], skats["scale_" + name]
    valid, padded, hd = (int(f[1:].lstrip("d")) for f in name.split("_")[:3])
    assert s.size == padded and scale == np.float32(1.0) / np.sqrt(np.float32(hd)) and s[0] == 0.0
    live = np.isfinite(s)
    assert np.all(s[~live] == -np.inf) and not live[valid:].any() and (live[:valid].all() or name.endswith("_holes")) and live[valid - 1]
    assert np.array_equal(s[live].astype(np.float16).astype(np.float32), s[live]) and np.all(s[live][1:] < 0)     # k_i . e_0 in an f16 cache gives them exactly
    e = ss.row_exps(po, s, scale)
    den = ss.row_denominators(e)
    inv_seq = np.float32(1.0 / den["seq"])
    assert inv_seq.view(np.uint32) == skats["inv_" + name].view(np.uint32)
    assert int(ss.dist(np.array([1.0 / den["seq"]]))[0]) <= ss.NEAR_UNITS == 8
    assert len(den) >= 3 and all(ss.guard_fires(t, padded) for t in den.values())
    assert list(skats["differs_" + name]) == sorted(n for n, t in den.items() if np.float32(1.0 / t).view(np.uint32) != inv_seq.view(np.uint32))
    # the oracle follows the reference: masked entries as a -inf mask on finite scores, as the attention builds them
    p = po.soft_max(np.where(live, s, 0).astype(np.float32), np.where(live, 0, -np.inf).astype(np.float32), scale)
    assert np.array_equal(p.view(np.uint32), (e * inv_seq).astype(np.float32).view(np.uint32))
