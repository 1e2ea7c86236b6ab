"""CPU: the case lists of tests/test_gpu_sweep_families.py (tests/family_cases.py) hold every class of shape the sweep exists for, so a later change of a seed or
of a list that drops one fails here, without a GPU; and, where the genuine reference is built (oracle/_ref/libggml_ref.so), the numpy restatements the sweep
takes its expectations from give the reference's bits at two of the widths the stored fixtures do not have."""
import numpy as np
import pytest

import family_cases as fc
import float_ref as fr
import iq4nl_ref as nl
import legacy1_ref as l1
import legacy_ref as lg
import lowbit_ref as lr
from bitcheck import assert_bits


# ---- restatements of the header expressions the classes come from -------------------------------------------------------------------------------------
def act_red_off(nb):
    """bamd_device.h: #define BAMD_ACT_RED_OFF(nb) ((((size_t) (nb) * (256 + 32 + 4)) + 15) & ~(size_t) 15)"""
    return (nb * (256 + 32 + 4) + 15) & ~15


def q0_split_nbuf(nb):
    """bamd_matvec_b32.h: constexpr int q0_split_nbuf(int nb) { return mv_terms_off(nb) + 2 * (size_t) nb * q0_term_floats * 4 <= (size_t) BAMD_LDS_CU_BYTES ? 2 : 1; }
    with bamd_mv_select.h: mv_terms_off(nb) = BAMD_ACT_RED_OFF(nb) + 16 * sizeof(double), BAMD_LDS_CU_BYTES = 160 * 1024 and
    bamd_b32_device.h: b32_term_floats(false) = 576"""
    return 2 if act_red_off(nb) + 16 * 8 + 2 * nb * 576 * 4 <= 160 * 1024 else 1


def q0_can_split(nb):
    """bamd_matvec_b32.h: constexpr bool q0_can_split(int nb) { return nb >= 8 && nb <= 56; }"""
    return 8 <= nb <= 56


def test_split_k_buffer_boundary_is_the_computed_one():
    two = [nb for nb in range(1, 100) if q0_can_split(nb) and q0_split_nbuf(nb) == 2]
    one = [nb for nb in range(1, 100) if q0_can_split(nb) and q0_split_nbuf(nb) == 1]
    assert two and one and max(two) + 1 == min(one), "the buffer count flips once inside q0_can_split"
    assert fc.SPLIT_NBUF_EDGE == (max(two), min(one))
    assert not q0_can_split(7) and q0_can_split(8) and q0_can_split(56) and not q0_can_split(57)
    assert set(fc.SPLIT_EDGES) == {7, 8, 9, 15, max(two), min(one), 56, 57}


def test_token_tile_switch_is_the_computed_one():
    """bamd_prefill_b32.h, launch_matmul_batch_b32: tt = (size_t) BAMD_TT * BAMD_BLOB_BYTES(a.K >> 8) <= 160 * 1024 ? BAMD_TT : 4, BAMD_BLOB_BYTES = BAMD_ACT_RED_OFF"""
    assert 8 * act_red_off(fc.TILE8_NB) <= 160 * 1024 < 8 * act_red_off(fc.TILE8_NB + 1)
    assert 4 * act_red_off(fc.TILE8_NB + 1) <= 160 * 1024          # the launcher takes the shape (tiles of 4)


# ---- the lists ---------------------------------------------------------------------------------------------------------------------------------------
def test_the_table_has_the_eleven_types():
    assert sorted(fc.TYPES) == sorted([10, 11, 8, 2, 6, 3, 7, 20, 1, 30, 0])
    for t, f in fc.FAMILIES.items():
        assert (2 in f.modes) == (t in fc.SPLIT_TYPES or t in (fc.Q2_K, fc.Q3_K))
        assert (f.switch is None) == (t == fc.BF16)


@pytest.mark.parametrize("t", fc.TYPES)
def test_mat_vec_cases_hold_every_class(t):
    cases = fc.matvec_cases(t)
    assert cases == fc.matvec_cases(t), "the list is deterministic"
    assert 8 <= len(cases) <= 16
    seen = set()
    for c in cases:
        assert c.K % 256 == 0 and c.rows >= 1
        seen |= fc.class_of(t, c.K // 256)
    nbs = [c.K // 256 for c in cases]
    assert any(nb == 1 for nb in nbs), "nb = 1"
    assert any(nb > 1 and nb & 1 for nb in nbs), "nb odd and greater than 1"
    assert any(nb > 2 and nb % 4 == 2 for nb in nbs), "nb = 2 (mod 4) and greater than 2: the depth-2 ring refills inside a row"
    assert any(nb % 4 == 0 for nb in nbs), "nb = 0 (mod 4)"
    if t in fc.SPLIT_TYPES:
        for nb in (7, 8, 9, 15) + fc.SPLIT_NBUF_EDGE + (56, 57):
            assert nb in nbs, "split-K edge nb = %d" % nb
    if t in (fc.F16, fc.BF16):
        assert any(nb > 1 and nb & 1 for nb in nbs), "an odd chunk count above 1 (a chunk of these types is 256 columns)"
    assert set(fc.classes(t)) <= seen
    assert any(c.rows % 8 for c in cases), "ragged rows"
    assert any(c.norm for c in cases) and any(not c.norm for c in cases), "RMSNorm on and off"
    assert any(c.resid for c in cases) and any(not c.resid for c in cases), "residual on and off"
    assert any(c.i % 5 == 0 for c in cases), "a case with an all-zero leading activation block"


@pytest.mark.parametrize("t", fc.TYPES)
def test_pair_and_batch_cases(t):
    for cases in (fc.gateup_cases(t), fc.argmax_cases(t)):
        assert len(cases) == 3 and all(c.rows % 8 for c in cases), "ragged rows throughout"
        nbs = [c.K // 256 for c in cases]
        assert any(nb > 2 and nb % 4 == 2 for nb in nbs) and any(nb > 1 and nb & 1 for nb in nbs)
    assert all(c.rows >= 63 for c in fc.argmax_cases(t)), "eight row-groups at least: the tie needs two workgroups"
    b = fc.batch_cases(t)
    nbs = [c.K // 256 for c in b]
    assert 4 <= len(b) <= 6 and all(c.T in fc.BATCH_T for c in b)
    assert any(nb > 2 and nb % 4 == 2 for nb in nbs) and any(nb > 1 and nb & 1 for nb in nbs)
    if t not in fc.FLOAT_TYPES:
        assert fc.TILE8_NB in nbs and fc.TILE8_NB + 1 in nbs, "both sides of the token-tile switch"
        # bamd_prefill_b32.h: if ((nb & 1) == 0 && !(MIN && PAIR && TT == 8) && !(BAMD_B32_MM_NL != 0 && TT == 8)) ... ring depth 2
        assert any(nb % 2 == 0 and 8 * act_red_off(nb) > 160 * 1024 for nb in nbs), "an even nb at token tiles of 4: ring depth 2 there, for IQ4_NL the only depth-2 launch"


def test_tall_cases_exceed_the_wave_slots():
    for t in fc.TYPES:
        cases = fc.tall_cases(t)
        assert {c.epi for c in cases} == {"add", "gateup", "argmax"}
        per_walk = 2 if t in fc.FLOAT_TYPES else 1
        for c in cases:
            walks = -(-c.nrg // per_walk)
            assert walks > fc.WAVE_SLOTS and c.rows == 8 * c.nrg - 3, "a wave walks twice; the last row-group is ragged"
        if t not in (fc.Q2_K, fc.Q3_K):
            assert {c.K for c in cases} == {256, 1024, 1536}
            assert any(-(-c.nrg // per_walk) > 2 * fc.WAVE_SLOTS for c in cases), "some waves walk three times"
        if t not in (fc.Q2_K, fc.Q3_K) + fc.FLOAT_TYPES:
            assert any(c.epi == "gateup" and c.K == 1536 for c in cases), "the pair epilogue across a row-group change with a ring of two slots"


def test_segment_cases_hold_every_boundary_class():
    cases = fc.segment_cases()
    assert cases == fc.segment_cases()
    forms = {c.form for c in cases}
    assert forms == {"q8_0", "q8_1", "f32", "q8_K", "bf16"}
    for form in forms:
        mine = [c for c in cases if c.form == form]
        assert {len(c.types) for c in mine} <= {2, 3} and all(len({fc.family(t).act for t in c.types}) == 1 for c in mine)
        nonlast = [r for c in mine for r in c.rows[:-1]]
        assert any(((r + 7) // 8) & 1 for r in nonlast), "%s: an odd row-group count in a non-last segment" % form
        assert any(r % 8 for r in nonlast), "%s: a ragged non-last segment" % form
        per = 2 if form in ("f32", "bf16") else 1
        assert any(min(c.rows) < 8 * fc.GRID * per < max(c.rows) for c in mine), "%s: a segment smaller than the grid beside a larger one" % form
        if form != "bf16":
            assert any(len(set(c.types)) > 1 for c in mine), "%s: mixed types" % form
    pure = [c for c in cases if all(t in fc.SPLIT_TYPES for t in c.types)]
    assert all(c.modes == (0, 1, 2) for c in pure)
    assert any(q0_can_split(c.K // 256) for c in pure) and any(not q0_can_split(c.K // 256) for c in pure), "mode 2 at a K inside and a K outside q0_can_split"
    # gap: matvec_q0_split_kernel's ctr carries across segments only where a workgroup owns row-groups of two segments
    carried = [c for c in pure if q0_can_split(c.K // 256) and sum((r + 7) // 8 for r in c.rows) > fc.GRID and any(len(set(w)) > 1 for w in fc.slot_segments(c.rows))]
    assert any(q0_split_nbuf(c.K // 256) == 2 and any(len(w) >= 3 for w in fc.slot_segments(c.rows)) for c in carried), "split-K, two term buffers: a workgroup walks three row-groups over two segments"
    assert any(q0_split_nbuf(c.K // 256) == 1 for c in carried), "split-K, one term buffer: a workgroup's walk spans two segments"
    assert all(len(set(c.types)) == 3 for c in carried)
    assert all(2 not in c.modes for c in cases if fc.IQ4_NL in c.types or c.form in ("q8_1", "f32", "bf16"))
    for a in (fc.Q8_0, fc.Q4_0, fc.Q5_0):
        assert any(fc.IQ4_NL in c.types and a in c.types for c in cases), "IQ4_NL beside type %d" % a


# ---- the restatements at widths the stored fixtures do not have, against the live reference ------------------------------------------------------------
WIDTHS = [1536, 5632]                            # nb = 6 and 22; the stored cases: K = 256, 512, 1024, 4096, 11008, 14336
ROWS = 32                                        # what every reference_outputs takes


def _inputs(t, K):
    rng = np.random.default_rng([77, t, K])
    W = fc.FAMILIES[t].gen(t, K, ROWS, rng)
    xs = [(rng.standard_normal(K) * s).astype(np.float32) for s in (1e-2, 1.0, 30.0)]
    return W, xs


@pytest.mark.parametrize("K", WIDTHS)
@pytest.mark.parametrize("t", fc.TYPES)
def test_restatement_equals_the_live_reference_at_new_widths(po, t, K):
    """ggml_vec_dot_* (and llamafile_sgemm where it serves the type) against the restatement's mul_mat, 32 rows, three activation magnitudes"""
    mod = lr if t in (fc.Q2_K, fc.Q3_K) else lg if t in fc.SPLIT_TYPES else l1 if t in (fc.Q4_1, fc.Q5_1) else nl if t == fc.IQ4_NL else fr
    L = mod.load_ref()
    if L is None:
        pytest.skip("oracle/_ref/libggml_ref.so is not built here")
    assert lg.ROWS == l1.ROWS == nl.ROWS == fr.ROWS == lr.ROWS == ROWS
    W, xs = _inputs(t, K)
    if mod is fr:
        out = fr.reference_outputs(L, t, W, xs)
        want = out["dots"] if t == fc.BF16 else out["sgemm1"]
    elif mod is nl:
        want = nl.reference_outputs(L, W, xs, (0,))[0]
    else:
        r = mod.reference_outputs(L, t, W, xs, (0,))
        want = r[0]
        if mod is lg and t in lg.SGEMM_TYPES:
            assert_bits(r[3], want, "llamafile_sgemm and ggml_vec_dot, type %d K %d" % (t, K))
    assert np.abs(want).max() > 0
    for i, x in enumerate(xs):
        assert_bits(fc.FAMILIES[t].ref(po, t, W, ROWS, K, x), want[i], "type %d K %d vector %d" % (t, K, i))
