"""CPU: the slice plan of a micro-batch's attention (bamd_attention_batch_plan, include/bamd.h) — which the launcher, the engine's scratch allocation and the
op-level entry point all go through — over a grid of (Hkv, gq, hd, T, ld, impl, budget).  Host code only: no device is opened.

What a plan must satisfy, whatever the shape:
  * slices are whole token tiles (16 / gq tokens on the matrix cores, 1 on the VALU), cover [0, T) exactly once, and the block fits the budget;
  * up to ld 18432 the default budget (0) gives ONE slice with the scratch size the matrix-core kernel took before the plan existed
    (Hkv x ceil(T / tt) x 16 x ld x 4 bytes beyond 512 positions at head_dim 128 and gq 1 / 2 / 4 / 8, else none);
  * a budget below one tile's workgroups is no plan (beyond the LDS), and the plan of a block sized by a plan is that plan again (the launcher re-plans from the
    block it is handed).
"""
import itertools

import pytest

import booster_amd

LDS_MAX = 144 * 1024
MFMA_GQ = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def plan():
    from booster_amd import build
    build.build()
    return booster_amd.attention_batch_plan


def on_mfma(gq, hd, T, impl):
    return impl != 1 and hd == 128 and T >= 2 and gq in MFMA_GQ


def tile_of(gq, hd, T, impl):
    return 16 // gq if on_mfma(gq, hd, T, impl) else 1


def per_tile_bytes(Hkv, gq, hd, T, ld, impl):
    if on_mfma(gq, hd, T, impl):
        return Hkv * 16 * ld * 4 if ld > 512 else 0
    return 0 if ld * 8 <= LDS_MAX else Hkv * gq * ld * 4


def legacy_scratch(Hkv, gq, hd, T, ld, impl):
    """what bamd_op_attention_batch allocated before the plan: bamd_attention_batch_mfma_scratch at head_dim 128 unless impl 1"""
    if hd != 128 or impl == 1 or ld <= 512 or gq not in MFMA_GQ or T < 2:
        return 0
    tt = 16 // gq
    return Hkv * ((T + tt - 1) // tt) * 16 * ld * 4


SHAPES = [(Hkv, gq, hd) for Hkv in (1, 2, 8) for gq in range(1, 9) for hd in (64, 128, 192, 256)]
TS = (1, 2, 5, 16, 37, 511, 512)
LDS = (64, 512, 576, 4096, 18432, 18496, 20480, 36928, 131072)


def check_plan(plan, Hkv, gq, hd, T, ld, impl, budget):
    r = plan(Hkv, gq, hd, T, ld, impl, budget)
    tt, pt = tile_of(gq, hd, T, impl), per_tile_bytes(Hkv, gq, hd, T, ld, impl)
    what = "Hkv %d gq %d hd %d T %d ld %d impl %d budget %d" % (Hkv, gq, hd, T, ld, impl, budget)
    if impl == 2 and not on_mfma(gq, hd, T, impl):
        assert r is None, what
        return None
    eff = budget or Hkv * gq * 512 * 18432 * 4
    if pt > eff:                                        # not one tile: no plan — except the VALU kernels with their rows in LDS, which need no block
        if ld * 8 <= LDS_MAX and impl == 0:
            assert r == (T, 1, 0), what
        else:
            assert r is None, what
        return r
    assert r is not None, what
    tps, ns, sb = r
    assert tps > 0 and tps % tt == 0, what
    assert sb == (tps // tt) * pt and sb <= eff, what
    # slices [i * tps, min(T, (i + 1) * tps)) cover [0, T) exactly once, none empty
    assert (ns - 1) * tps < T <= ns * tps, what
    ntiles = (T + tt - 1) // tt
    if pt:
        assert ns == -(-ntiles // min(ntiles, eff // pt)), what          # no more slices than the budget forces
        assert tps // tt == -(-ntiles // ns), what                       # balanced
    else:
        assert ns == 1 and sb == 0, what
    return r


@pytest.mark.parametrize("impl", [0, 1, 2])
def test_default_budget(plan, impl):
    for (Hkv, gq, hd), T, ld in itertools.product(SHAPES, TS, LDS):
        r = check_plan(plan, Hkv, gq, hd, T, ld, impl, 0)
        if r is not None and ld <= 18432:
            tt = tile_of(gq, hd, T, impl)
            assert r == ((T + tt - 1) // tt * tt, 1, legacy_scratch(Hkv, gq, hd, T, ld, impl)), (Hkv, gq, hd, T, ld, impl, r)


@pytest.mark.parametrize("impl", [0, 1, 2])
def test_budgets(plan, impl):
    for (Hkv, gq, hd), T, ld in itertools.product(SHAPES[::3], TS, LDS):
        pt = per_tile_bytes(Hkv, gq, hd, T, ld, impl)
        for budget in (1, 4096, pt - 1, pt, pt + 1, 2 * pt + 7, 3 * pt, 5 * pt - 1, 1 << 40):
            if budget > 0:
                check_plan(plan, Hkv, gq, hd, T, ld, impl, budget)


def test_budget_below_one_tile_fails(plan):
    """beyond the LDS a block that cannot hold one tile's workgroups for every KV head is no plan (the engine then goes token by token)"""
    for Hkv, gq, hd, impl in ((8, 4, 128, 0), (8, 4, 128, 2), (2, 3, 128, 0), (1, 8, 64, 1), (4, 1, 256, 0)):
        ld = 20480
        pt = per_tile_bytes(Hkv, gq, hd, 37, ld, impl)
        assert pt > 0
        assert plan(Hkv, gq, hd, 37, ld, impl, pt - 1) is None
        tps, ns, sb = plan(Hkv, gq, hd, 37, ld, impl, pt)
        tt = tile_of(gq, hd, 37, impl)
        assert (tps, ns, sb) == (tt, (37 + tt - 1) // tt, pt)


def test_slices_are_balanced_and_stable(plan):
    """10 tiles under a budget of 9: two slices of 5 tiles, not 9 + 1; and the plan of the resulting block is the same plan"""
    Hkv, gq, hd, ld = 2, 4, 128, 18624
    pt = per_tile_bytes(Hkv, gq, hd, 40, ld, 0)
    assert plan(Hkv, gq, hd, 40, ld, 0, 9 * pt) == (20, 2, 5 * pt)
    for T, fit in itertools.product((5, 29, 37, 100, 512), (1, 2, 3, 7, 100)):
        for g, h, impl in ((4, 128, 0), (3, 128, 0), (8, 64, 1)):
            p1 = plan(Hkv, g, h, T, ld, impl, fit * per_tile_bytes(Hkv, g, h, T, ld, impl))
            assert plan(Hkv, g, h, T, ld, impl, p1[2]) == p1


def test_bad_shapes_have_no_plan(plan):
    for args in ((0, 4, 128, 8, 1024), (2, 0, 128, 8, 1024), (2, 9, 128, 8, 1024), (2, 4, 96, 8, 1024), (2, 4, 320, 8, 1024), (2, 4, 128, 0, 1024),
                 (2, 4, 128, 8, 1000), (2, 4, 128, 8, 0)):
        assert plan(*args, 0, 0) is None, args
    assert plan(2, 4, 128, 8, 1024, 3, 0) is None
