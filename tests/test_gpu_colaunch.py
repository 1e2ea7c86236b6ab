"""GPU: the co-launched attention + wo kernel (csrc/bamd_colaunch.hip) called directly through bamd_op_attention_wo, which fills the argument blocks as
the decode step does and calls the same launcher.  Expectation: oracle_attention (decode semantics) for the attention output, then residual + mul_mat of
the wo matrix on it (the oracle's mul_mat_q for Q4_K / Q5_K / Q6_K, tests/lowbit_ref.py for Q2_K / Q3_K).  Compared on raw bits: x2, the value half of
every granule against the attention output, the tag half against (serial << 20) | ((step & 0xfff) << 8) | il, both caches; the give-up counter must be 0.
Every expectation is finite (the finiteness rule of tests/edge_inputs.py).

A launch in which the attention role never publishes is NOT built here: the give-up path is a bounded one-second spin and is not to be provoked.

The serial-wrap guard of the engine (next_serial) is tested at the end through the public API."""
import os

import numpy as np
import pytest

import edge_inputs as ei
import lowbit_ref as lr
from booster_amd import gguf
from bitcheck import bits
from booster_amd.gguf import random_kquant_tensor
from test_gpu_ops import oracle_attention

gpu = pytest.mark.gpu
K = 4096
TYPES = [12, 13, 14, 11, 10]                        # Q4_K, Q5_K, Q6_K, Q3_K, Q2_K
LAYOUTS = [(32, 8, 128), (32, 32, 128), (32, 4, 128), (64, 8, 64), (16, 2, 256), (16, 16, 256)]      # H * hd = 4096
POSITIONS = [0, 31, 32, 63, 64, 255, 256, 383, 446, 447]
ROW_KINDS = ("extra0", "4096", "extra_max", "ragged")
SERIALS, STEPS, ILS = (1, 0xffe), (0, 0xfff, 0x1000, 0x12345), (0, 255)
GRAN_KINDS = ("zero_tag", "ff", "il-1", "step-1", "serial-1")
NAN_BITS = 0x7fc00000
# activation kinds of tests/edge_inputs.py fed through v.  The V cache is f16: `tiny_max` and `overflow_iscale` blocks (maxima of 1e-30 and 1e-37) would
# round to zeros on the way, and the magnitudes of `huge` and `single` do not fit, so those four edges of the quantiser cannot be reached through this launch
EDGE_AKINDS = ("random", "zero", "constant", "near_constant", "ties", "opposite_max")


def tag_of(serial, step, il):
    return ((serial << 20) | ((step & 0xfff) << 8) | il) & 0xffffffff


def plan():
    """the cases of test_types_layouts_positions: every type meets every layout, and the positions are dealt so that every position meets every head size
    (one per case; two where a head size has one layout only); rows, tag and initial granules cycle along"""
    cases, n_of_hd = [], {}
    for li, (H, Hkv, hd) in enumerate(LAYOUTS):
        for ti, t in enumerate(TYPES):
            i = n_of_hd.get(hd, 0); n_of_hd[hd] = i + 1
            j = len(cases)
            positions = (POSITIONS[(2 * i) % 10], POSITIONS[(2 * i + 1) % 10]) if hd == 64 else (POSITIONS[i % 10],)
            cases.append(dict(t=t, H=H, Hkv=Hkv, hd=hd, positions=positions, rows=ROW_KINDS[(li + ti) % 4],
                              serial=SERIALS[j % 2], step=STEPS[(j // 2) % 4], il=ILS[(j // 8) % 2], gran=(None, "ff") if j % 2 else ("ff", None)))
    return cases


def test_plan_covers_the_cross_product():
    cases = plan()
    assert {(c["t"], c["H"], c["Hkv"], c["hd"]) for c in cases} == {(t,) + l for t in TYPES for l in LAYOUTS}
    assert {(p, c["hd"]) for c in cases for p in c["positions"]} == {(p, hd) for p in POSITIONS for hd in (64, 128, 256)}
    assert {c["rows"] for c in cases} == set(ROW_KINDS)


def ref_mul_mat(po, t, W, rows, x):
    if t in (lr.Q2_K, lr.Q3_K):
        return lr.mul_mat(po, t, W, rows, K, x)
    return po.mul_mat_q(t, W, rows, K, x, nthreads=8)[0]


def wo_rows(kind, n_cu, H):
    """wo row counts at the edges of `extra` = row-groups - 2 G, G = the CUs the wo role has: the first `extra` workgroups take a third row-group"""
    G = n_cu - H
    return {"extra0": 16 * G, "4096": 4096, "extra_max": 24 * G - 8, "ragged": 4090}[kind]


def initial_granules(kind, n, serial, step, il, rng):
    """what the granules hold before the launch: the value halves a NaN bit pattern (a granule consumed before it is published poisons x2), the tag halves
    zero, all-ones, or the tag of the neighbouring use"""
    if kind is None:
        return None
    if kind == "ff":
        return np.full(n, 0xffffffffffffffff, np.uint64)
    val = (NAN_BITS | rng.integers(0, 1 << 22, n)).astype(np.uint64)
    tag = {"zero_tag": 0, "il-1": tag_of(serial, step, il - 1), "step-1": tag_of(serial, step - 1, il), "serial-1": tag_of(serial - 1, step, il)}[kind]
    assert tag != tag_of(serial, step, il)
    return val | (np.uint64(tag) << np.uint64(32))


_cus = []


def device_cus(bamd):
    """the CU count the op hands the launcher (reported by a call the launcher declines: K = 2048)"""
    if not _cus:
        z = np.zeros
        r = bamd.op_attention_wo(z(2048, np.float32), z(512, np.float32), z(512, np.float32), z(64 * 512, np.uint16), z(64 * 512, np.uint16), z(128, np.float32),
                                 16, 4, 128, 64, 0, 12, z(8 * 8 * 144, np.uint8), 8, z(8, np.float32))
        assert r["declined"], "K = 2048 has no co-launch kernel"
        _cus.append(r["n_cu"])
    return _cus[0]


def attention_inputs(rng, H, Hkv, hd, n_ctx):
    Ekv = Hkv * hd
    kc = (rng.standard_normal(n_ctx * Ekv) * 0.7).astype(np.float16).view(np.uint16).copy()
    vc = rng.standard_normal(Ekv * n_ctx).astype(np.float16).view(np.uint16).copy()
    q = (rng.standard_normal(H * hd) * 2).astype(np.float32)
    k = rng.standard_normal(Ekv).astype(np.float32)
    v = rng.standard_normal(Ekv).astype(np.float32)
    return q, k, v, kc, vc


def run_case(bamd, po, t, H, Hkv, hd, n_ctx, pos, rows, lds_ld=0, serial=1, step=1, il=0, gran_kind=None, seed=0, v=None, W=None, what="", ref=ref_mul_mat):
    """one co-launch against the oracle; rows: a row count or one of ROW_KINDS; ref(po, t, W, rows, x): the reference mat-mul of the wo rows"""
    what = "%s type %d H %d Hkv %d hd %d n_ctx %d lds_ld %d pos %d rows %s tag (%#x, %#x, %d) granules %s" % (what, t, H, Hkv, hd, n_ctx, lds_ld, pos, rows, serial, step, il, gran_kind)
    if os.environ.get("BAMD_COLAUNCH") == "0":
        pytest.skip("the co-launch is switched off by the environment (BAMD_COLAUNCH=0)")
    n_cu = device_cus(bamd)
    if isinstance(rows, str):
        rows = wo_rows(rows, n_cu, H)
    if n_cu != 256 and ((rows + 7) // 8) // (n_cu - H) != 2:
        pytest.skip("%d CUs: %d row-groups over the %d wo workgroups is not two or three each, the launcher declines by design" % (n_cu, (rows + 7) // 8, n_cu - H))
    rng = np.random.default_rng([seed, t, H, Hkv, hd, pos, rows])
    q, k, v0, kc, vc = attention_inputs(rng, H, Hkv, hd, n_ctx)
    v = v0 if v is None else v
    if W is None:
        W = random_kquant_tensor(t, K, rows, rng)
    res = rng.standard_normal(rows).astype(np.float32)
    rope = po.rope_cache(pos, hd, 500000.0)
    kc2, vc2 = kc.copy(), vc.copy()
    att, _ = oracle_attention(po, q, k, v, kc2, vc2, rope, H, Hkv, hd, n_ctx, pos, False)
    want = ref(po, t, W, rows, att) + res
    assert np.isfinite(att).all() and np.isfinite(want).all(), what + ": the expectation is not finite"
    g0 = initial_granules(gran_kind, H * hd, serial, step, il, rng)
    r = bamd.op_attention_wo(q, k, v, kc, vc, rope, H, Hkv, hd, n_ctx, pos, t, W, rows, res, lds_ld=lds_ld, serial=serial, step=step, il=il, gran_init=g0)
    assert not r["declined"], what + ": the launcher declined a shape it must accept (%d CUs)" % n_cu
    assert r["gave_up"] == 0, what + ": a wo workgroup gave up waiting"
    gran = r["gran"]
    tags = (gran >> np.uint64(32)).astype(np.uint32)
    bad = np.flatnonzero(tags != tag_of(serial, step, il))
    assert bad.size == 0, "%s: attention role, %d granule tags differ, first at %d (head %d): %#x, want %#x" % (what, bad.size, bad[0], bad[0] // hd, tags[bad[0]], tag_of(serial, step, il))
    vals = (gran & np.uint64(0xffffffff)).astype(np.uint32)
    bad = np.flatnonzero(vals != bits(att))
    assert bad.size == 0, "%s: attention role, %d granule values differ, first at %d (head %d): %r vs %r" % (what, bad.size, bad[0], bad[0] // hd, vals[bad[0]:bad[0] + 1].view(np.float32)[0], att[bad[0]])
    assert np.array_equal(kc, kc2), what + ": K cache differs"
    assert np.array_equal(vc, vc2), what + ": V cache differs"
    bad = np.flatnonzero(bits(r["x2"]) != bits(want))
    assert bad.size == 0, "%s: wo role, %d/%d rows differ, first row %d: %r vs %r" % (what, bad.size, rows, bad[0], r["x2"][bad[0]], want[bad[0]])
    return r


# ---- every type x every head layout, every position x every head size -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("c", plan(), ids=lambda c: "t%d-H%d-Hkv%d-hd%d" % (c["t"], c["H"], c["Hkv"], c["hd"]))
def test_types_layouts_positions(bamd, po, c):
    """n_ctx 512 with 512-float LDS rows; positions up to 447 (the last one the engine co-launches), among them 256 .. 447: the K / V^T tiles beyond the four
    requested at entry"""
    for pos, gk in zip(c["positions"], c["gran"]):
        run_case(bamd, po, c["t"], c["H"], c["Hkv"], c["hd"], 512, pos, c["rows"], lds_ld=512, serial=c["serial"], step=c["step"], il=c["il"], gran_kind=gk)


# ---- n_ctx / lds_ld pairs ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n_ctx,lds_ld,positions,t", [(96, 128, (31, 95), 12), (96, 128, (31, 95), 14), (128, 128, (64, 127), 13), (128, 128, (64, 127), 11),
                                                       (4096, 512, (255, 446), 14), (4096, 512, (255, 446), 10), (4096, 0, (32, 383), 12), (4096, 0, (32, 383), 13)])
def test_context_and_lds_row_lengths(bamd, po, t, n_ctx, lds_ld, positions):
    """short contexts (LDS rows = the padded n_ctx; 96 is padded to 128) and the engine's large-context case: V^T rows of stride 4096 against LDS rows of 512
    (lds_ld 0 = the op's own min(512, padded n_ctx), as the engine passes it)"""
    for pos in positions:
        run_case(bamd, po, t, 32, 8, 128, n_ctx, pos, 4096, lds_ld=lds_ld, serial=3, step=pos + 1, il=t)


# ---- wo row counts at the edges of `extra` ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("t,rows", [(t, r) for t in (12, 13, 14) for r in ROW_KINDS] + [(11, "ragged"), (11, "extra_max"), (10, "extra0"), (10, "4096")])
def test_wo_row_counts(bamd, po, t, rows):
    """16 G rows (no workgroup takes a third row-group), 4096, 24 G - 8 (all but one do), 4090 (nvalid < nrows: a ragged last row-group)"""
    run_case(bamd, po, t, 32, 8, 128, 512, 37, rows, lds_ld=512)


@gpu
@pytest.mark.parametrize("H,Hkv,hd,t,rows", [(64, 8, 64, 13, r) for r in ROW_KINDS] + [(16, 2, 256, 14, r) for r in ROW_KINDS] +
                         [(64, 8, 64, 11, "extra_max"), (16, 2, 256, 10, "ragged")])
def test_wo_row_counts_other_grids(bamd, po, H, Hkv, hd, t, rows):
    """the same with 64 and 16 attention workgroups: G = CUs - H changes, and with it every row-group's owner"""
    run_case(bamd, po, t, H, Hkv, hd, 512, 70, rows, lds_ld=512)


# ---- tags ---------------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("il", ILS)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("serial", SERIALS)
def test_tags(bamd, po, serial, step, il):
    """the last serial before the wrap, steps at and beyond the 12 bits of the tag's step field, the last layer index"""
    run_case(bamd, po, (12, 14)[(step + il) % 2], 32, 8, 128, 512, 40, 4096, lds_ld=512, serial=serial, step=step, il=il)


# ---- what the granules hold before the launch ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("t,kind", [(12, k) for k in GRAN_KINDS] + [(13, "ff"), (14, "il-1"), (11, "step-1"), (10, "serial-1")])
def test_initial_granules(bamd, po, t, kind):
    """NaN values under a tag that is not this launch's — zero, all-ones, the previous layer's, the previous step's, the previous host call's: the wo role
    must wait for every granule of its slice, or x2 is NaN"""
    run_case(bamd, po, t, 32, 8, 128, 512, 65, "extra_max", lds_ld=512, serial=7, step=0x123, il=9, gran_kind=kind)


# ---- value edges through the wo role's own quantiser --------------------------------------------------------------------------------------------------
def edge_values(rng):
    """edge activations (tests/edge_inputs.py) for the wo role, fed through v: every block scaled by a power of two (which keeps ties, constants and
    opposite maxima what they are) until its magnitudes fit f16"""
    x, tags = ei.edge_activations(K, rng, kinds=EDGE_AKINDS)
    x = x.reshape(-1, 256).copy()
    for b in x:
        m = np.abs(b).max()
        if m > 32768.0:
            b *= np.float32(2.0 ** -int(np.ceil(np.log2(m / 32768.0))))
    return x.reshape(-1), tags


def first_position_attention(po, v, H, hd, seed):
    """the oracle's attention at position 0 with one query head per KV head: (att, the other inputs)"""
    rng = np.random.default_rng(seed)
    q, k, _, kc, vc = attention_inputs(rng, H, H, hd, 64)
    att, _ = oracle_attention(po, q, k, v, kc.copy(), vc.copy(), po.rope_cache(0, hd, 500000.0), H, H, hd, 64, 0, False)
    return att


@pytest.mark.parametrize("H,hd", [(32, 128), (16, 256)])
def test_first_position_passes_v_through(po, H, hd):
    """the construction test_value_edges relies on, on the oracle alone: at position 0 the softmax row is (1, 0, ...), so with one query head per KV head
    the attention output is the f16 rounding of v — bit for bit, but for the sign of zero: every output is a chain 0 + v * 1 + c * 0 + ..., and
    (+0) + (-0) is +0.  What this construction carries to the quantiser: zero blocks, constant blocks, exact ties and opposite maxima"""
    rng = np.random.default_rng(hd)
    v, tags = edge_values(rng)
    assert set(tags) == set(EDGE_AKINDS)
    att = first_position_attention(po, v, H, hd, 5)
    v16 = v.astype(np.float16).astype(np.float32)
    assert np.isfinite(v16).all()
    assert np.array_equal(bits(att), bits(v16 + np.float32(0.0)))
    # what reaches the quantiser still holds the edges: all-zero blocks, a constant block (every quant -127), opposite maxima, exact .5 ties
    blk = att.reshape(-1, 256)
    assert (np.abs(blk).max(axis=1) == 0).sum() == sum(k == "zero" for k in tags) >= 2
    q8 = ei.q8_fields(po.quantize_q8_K(att))[1]
    assert any((row == -127).all() for row in q8)
    assert any((b.max() == -b.min()) and b.max() > 0 for b in blk)
    d = ei.q8_fields(po.quantize_q8_K(att))[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        scaled = blk.astype(np.float64) / d.astype(np.float64)[:, None]
    assert np.count_nonzero(np.isfinite(scaled) & (np.abs(scaled - np.trunc(scaled)) == 0.5)) >= 100


@gpu
@pytest.mark.parametrize("t,H,hd", [(t, H, hd) for t in (12, 13, 14) for H, hd in ((32, 128), (16, 256))] + [(11, 32, 128), (10, 16, 256)])
def test_value_edges(bamd, po, t, H, hd):
    """edge activations reach ActPro<false>::quantize_batch of the wo role as their f16 roundings (test_first_position_passes_v_through: zero blocks, a
    constant block, exact ties, opposite maxima), against edge weights for the types
    tests/edge_inputs.py covers"""
    rng = np.random.default_rng(100 * t + hd)
    v, _ = edge_values(rng)
    W = ei.edge_kquant_tensor(t, K, 4096, rng)[0] if t in ei.BLOCK_BYTES else None
    r = run_case(bamd, po, t, H, H, hd, 64, 0, 4096, lds_ld=64, serial=2, step=1, il=1, gran_kind="il-1", v=v, W=W, seed=t)
    v16 = v.astype(np.float16).astype(np.float32) + np.float32(0.0)
    assert np.array_equal((r["gran"] & np.uint64(0xffffffff)).astype(np.uint32), bits(v16))


# ---- shapes the launcher must refuse ------------------------------------------------------------------------------------------------------------------
@gpu
def test_declines(bamd, po):
    """K = 2048 has no co-launch instance, and shifted cells (a cell-position table) take the three-launch path: the launcher must say so, not launch"""
    assert device_cus(bamd) > 0                                   # (the K = 2048 call, asserted inside)
    rng = np.random.default_rng(9)
    q, k, v, kc, vc = attention_inputs(rng, 32, 8, 128, 512)
    W = random_kquant_tensor(12, K, 4096, rng)
    r = bamd.op_attention_wo(q, k, v, kc, vc, po.rope_cache(5, 128, 500000.0), 32, 8, 128, 512, 5, 12, W, 4096, np.zeros(4096, np.float32), with_cellpos=True)
    assert r["declined"]


# ---- the serial-wrap guard, through the public API ----------------------------------------------------------------------------------------------------
SERIAL_PERIOD = 0xffe                                # next_serial (csrc/bamd_engine.cpp): the host serial runs 1 .. 0xffe
_wrap_want = []


@gpu
@pytest.mark.parametrize("aql", [True, False])
def test_serial_wrap_clears_stale_granules(bamd, po, tmp_path, aql):
    """A one-layer model at the 8B widths.  decode([a], p) co-launches and leaves a's attention output in the granules under the tag (serial S, step 1,
    layer 0).  Single-token decodes at position 500 take the three-launch path: each takes the next serial and none touches the granules.  After
    SERIAL_PERIOD - 1 of them the next call carries serial S again, and decode([b], p) waits for exactly the tag the stale granules hold: without the
    0xff fill of next_serial at the wrap its wo role reads a's values and the logits are wrong.  That the probe lands on the right call was shown once
    on an MI355X with a build from which only that hipMemsetAsync was removed: both cases of this test failed at the last assertion with all 1024
    logits different (first logit 3.3491697 against 0.89251435), a wrong result and no fault; with the fill both pass.
    Expectation: the logits of the same decode([b], p) on the fresh context, themselves held to the oracle's model forward."""
    if os.environ.get("BAMD_COLAUNCH") == "0":
        pytest.skip("the co-launch is switched off by the environment (BAMD_COLAUNCH=0)")
    path = str(tmp_path / "wrap.gguf")
    gguf.write_synthetic_llama(path, E=4096, H=32, Hkv=8, L=1, F=1024, V=1024, seed=23)
    n_ctx, p, a, b = 1024, 300, 77, 901
    prompt = [(7919 * i + 13) % 1024 for i in range(512)]
    if not _wrap_want:                                # the same model and calls for both queues: one oracle run
        om = po.OracleModel(gguf.GGUFReader(path)); oc = po.OracleContext(om, n_ctx, nthreads=8)
        oc.decode(prompt, 0)
        _wrap_want.append(oc.decode([b], p))
        oc.close()
    want = _wrap_want[0]
    assert np.isfinite(want).all()
    bamd.set_aql(aql)
    try:
        m = bamd.Model(path); ctx = bamd.Context(m, n_ctx)
        ctx.decode(prompt, 0)
        first = ctx.decode([b], p)
        assert np.array_equal(bits(first), bits(want)), "decode([b], p) on the fresh context differs from the oracle"
        stale = ctx.decode([a], p)
        assert not np.array_equal(bits(stale), bits(want))
        for i in range(SERIAL_PERIOD - 1):
            ctx.decode([(a + i) % 1024], 500)
        again = ctx.decode([b], p)
        bad = np.flatnonzero(bits(again) != bits(want))
        assert bad.size == 0, "after the serial wrap %d/%d logits differ, first at %d: %r vs %r" % (bad.size, want.size, bad[0], again[bad[0]], want[bad[0]])
        if aql:
            assert ctx.aql_runs() > SERIAL_PERIOD, "the steps did not run on the own queue"
        ctx.close(); m.close()
    finally:
        bamd.set_aql(True)
