"""CPU: tests/sampler_ref.py held to account — its restatement of the sampler prefilter against the genuine sampler's fixtures (tests/golden/janus_kats.npz,
recorded from cpp/janus.cpp) and against the library's full-sort shortlist, and its case lists against what they promise, so that tests/test_gpu_sampler.py
cannot pass on subtly wrong arithmetic."""
import ctypes as C
import os

import numpy as np
import pytest

import booster_amd
import sampler_ref as sr
from booster_amd import gguf
from janus_cases import N_LAST, case_logits, digest

KATS = os.path.join(os.path.dirname(__file__), "golden", "janus_kats.npz")
EOS = 2                                                                  # cpp/janus.h:18
LANG_EN, LANG_RU, SPACE_RU, LANG_OTHER = 2, 3, 30, 4                      # cpp/janus.h token classes


@pytest.fixture(scope="module")
def L():
    lib = booster_amd.lib()
    lib.bamd_vocab_load.restype = C.c_void_p; lib.bamd_vocab_load.argtypes = [C.c_char_p]
    lib.bamd_vocab_free.argtypes = [C.c_void_p]
    lib.bamd_janus_test_new.restype = C.c_void_p
    lib.bamd_janus_test_new.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int]
    lib.bamd_janus_test_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bamd_janus_test_free.argtypes = [C.c_void_p]
    lib.bamd_janus_shortlist_test.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int]
    return lib


def full_sort_ids(L, logits, cutoff):
    """the id set of the library's full-sort shortlist (janus.cpp:285-324 as written: sort everything, cut at the first quotient below the cut-off)"""
    lg = np.ascontiguousarray(logits, np.float32)
    ids = np.zeros(lg.size, np.int32)
    n = L.bamd_janus_shortlist_test(lg.ctypes.data_as(C.c_void_p), lg.size, float(cutoff), 0, ids.ctypes.data_as(C.c_void_p), lg.size)
    assert 0 < n <= lg.size
    return np.sort(ids[:n])


def witness_applies(e):
    """the full sort says the same as the ratio set where the quotient is monotone along the sorted order: a unique positive top, no NaN"""
    return e["nan"] == 0 and e["ntop"] == 1 and e["top_logit"] is not None and e["top_logit"] > 0


def janus_penalties(types, scales, last, prompt_len, pos, n_max, depth, V):
    """the penalty list of one draw the way the bridge's device sampler builds it: the EOS `pre`, then one entry per distinct recent token with its
    multiplicity and kind; and the halve switch"""
    ru = types[last[-1]] in (SPACE_RU, LANG_RU)
    order, ent = [], {}

    def entry(i):
        if i not in ent:
            ent[i] = dict(id=i, count=0, kind=0, f=np.float32(1.0), d=1.0, pre=0.0); order.append(i)
        return ent[i]
    if V > EOS:
        entry(EOS)["pre"] = sr.janus_pre(pos - prompt_len, n_max)
    for i in range(min(int(depth), pos - prompt_len)):
        t = int(last[len(last) - 1 - i]); e = entry(t)
        if ru and types[t] == LANG_RU:
            e["kind"] = 1; e["d"] = 1.0 - (1.0 - float(scales[t])) * 0.20
        else:
            e["kind"] = 0; e["f"] = scales[t]
        e["count"] += 1
    pen = np.zeros(len(order), sr.PEN_DTYPE)
    for k, i in enumerate(order):
        e = ent[i]; pen[k] = (e["id"], e["count"], e["kind"], e["f"], e["d"], e["pre"])
    return pen, int(ru)


def check_fixture_set(L, name, tmp_path):
    """asserts what test_restatement_equals_genuine_sampler states; returns what the set exercised"""
    k = np.load(KATS)
    g = lambda key: k[name + "_" + key]
    V = int(g("V")[0]); scale, hi, lo, depth = g("params")
    path = str(tmp_path / "janus.gguf")
    gguf.write_synthetic_llama(path, E=256, H=2, Hkv=1, L=1, F=256, V=V, seed=3, vocab=gguf.synthetic_janus_vocab(V))
    vh = L.bamd_vocab_load(path.encode())
    assert vh
    j = L.bamd_janus_test_new(vh, float(scale), float(hi), float(lo), int(depth))
    try:
        types = np.zeros(V, np.float32); scales = np.zeros(V, np.float32)
        L.bamd_janus_test_tables(j, types.ctypes.data_as(C.c_void_p), scales.ctypes.data_as(C.c_void_p))
    finally:
        L.bamd_janus_test_free(j); L.bamd_vocab_free(vh)
    halve_class = ((types == LANG_EN) | (types == LANG_OTHER)).astype(np.uint8)
    n = len(g("token")); kinds, multi, pres, halved, witnessed = set(), 0, 0, 0, 0
    for c in range(n):
        logits = case_logits(g("seed")[c], V, g("negative")[c], g("ov_ids")[c], g("ov_vals")[c])
        last = np.ascontiguousarray(g("last")[c], np.int32)
        assert last.size == N_LAST
        pen, halve = janus_penalties(types, scales, last, int(g("prompt_len")[c]), int(g("pos")[c]), int(g("max")[c]), depth, V)
        assert np.unique(pen["id"]).size == pen.size
        after = sr.apply_penalties(logits, pen, halve_class, halve)
        assert digest(after) == str(g("digest")[c]), "case %d: logits after the penalties" % c
        kinds |= set(int(x) for x in pen["kind"][pen["count"] > 0]); multi += int((pen["count"] > 1).any()); pres += int((pen["pre"] != 0).any() and pen["pre"][0] != 1.0)
        halved += halve
        for cut in (hi, lo):
            e = sr.shortlist(after, np.full(V, cut, np.float32))
            if witness_applies(e):
                assert np.array_equal(e["ids"], full_sort_ids(L, after, cut)), "case %d cut-off %s" % (c, cut)
                witnessed += 1
    return kinds, multi, pres, halved, witnessed


@pytest.mark.parametrize("name", ["l2", "l2b", "l3"])
def test_restatement_equals_genuine_sampler(L, name, tmp_path):
    """apply_penalties on the bridge-style penalty list reproduces the genuine sampler's logits after the penalties (the fixture's digest), and shortlist() of
    them is the full sort's set at either cut-off of the fixture"""
    check_fixture_set(L, name, tmp_path)


def test_fixtures_exercise_the_restatement(L, tmp_path):
    """between them the fixture sets use both penalty kinds, repeated tokens, an EOS factor other than 1, the x0.5 pass and the full-sort witness"""
    tot = [set(), 0, 0, 0, 0]
    for name in ("l2", "l2b", "l3"):
        d = tmp_path / name; d.mkdir()
        r = check_fixture_set(L, name, d)
        tot[0] |= r[0]
        for i in range(1, 5):
            tot[i] += r[i]
    assert tot[0] == {0, 1} and min(tot[1:]) >= 1, tot


def witness_cases(V):
    """every case of the size, but of class A at the Llama-3 size only every 16th position and the array's ends (a full sort of 128256 logits per case)"""
    cs = sr.cases(V)
    return [c for i, c in enumerate(cs) if not (V > 5000 and c.cls == "A" and i % 16 and c.name not in ("top@0", "top@%d" % (V - 1)))]


@pytest.mark.parametrize("V", sr.VS)
def test_restatement_equals_full_sort_on_the_cases(L, V):
    n = 0
    for c in witness_cases(V):
        after, e = c.expect()
        if witness_applies(e):
            assert np.array_equal(e["ids"], full_sort_ids(L, after, e["cutoff"])), c
            n += 1
        else:
            assert c.cls not in "ABCH", c                                # these classes promise a unique positive top and no NaN
    assert n >= 20


@pytest.mark.parametrize("V", sr.VS)
def test_expectations_are_not_trivial(V):
    cs = sr.cases(V)
    classes = set(c.cls for c in cs)
    assert classes == set("ABDEFGH") | (set("C") if V >= 4100 else set())
    pos = set(sr.top_positions(V))
    assert [c.name for c in cs if c.cls == "A"] == ["top@%d" % p for p in sorted(pos)]
    for b in list(range(64, V, 64)) + list(range(1024, V, 1024)):
        assert b - 1 in pos and b in pos
    assert 0 in pos and V - 1 in pos
    cls, cut, base = sr.tables(V)
    assert 0.25 < cls.mean() < 0.35 and set(np.unique(cut)) == {sr.CUT_HI, sr.CUT_LO}
    for c in cs:
        before = c.logits(); after, e = c.expect()
        changed = np.nonzero(before.view(np.uint32) != after.view(np.uint32))[0]
        if c.cls in sr.COLLECTING:
            assert e["count"] > 1 and e["nan"] == 0 and e["top_logit"] > 0, c
        if c.cls in "ABC":
            assert e["ntop"] == 1 and changed.size == 0, c
        if c.cls == "A":
            assert e["top_id"] == int(c.name[4:]), c
        if c.cls == "C":                                                 # the cap cases hit their counts exactly
            assert e["count"] == c.meta["n"], c
        if c.cls == "D":
            assert e["ntop"] == c.meta["ntop"] and e["top_id"] == 5 and set((5, V - 1)) <= set(e["ids"]), c
            assert (after == np.nextafter(np.float32(12.0), np.float32(0.0))).sum() == 1, c      # an ulp below the ties: a candidate, not one of them
        if c.cls == "E":
            assert e["count"] == 0 and e["ntop"] == 0 and not (e["top_logit"] > 0), c
        if c.cls == "F":
            nan_ids = np.nonzero(np.isnan(after))[0]
            assert e["nan"] == 1 and nan_ids.size == c.meta["n_nan"], c
            if c.name == "all":
                assert e["top_id"] == -1 and e["count"] == 0 and np.unique(after.view(np.uint32)).size == 3
            else:
                assert e["top_logit"] == 12.0 and set(nan_ids) <= set(e["ids"]) and e["count"] > nan_ids.size + 1, c
        if c.cls == "H":
            assert e["top_id"] == c.meta["top"] and e["ntop"] == 1, c
            assert set(changed) <= set(c.pen["id"]) | (set(np.nonzero(c.halve_class)[0]) if c.halve else set()), c
            if c.pen.size == 0 and not c.halve:
                assert changed.size == 0
            if c.halve:
                assert after[c.meta["top"]] == 10.0 and changed.size > 0.25 * V, c
                if c.name == "halve-dethrones":                          # the top before the pass is halved and loses to one that is not
                    w = c.meta["was_top"]
                    assert before[w] == before.max() and c.halve_class[w] and not c.halve_class[c.meta["top"]] and after[w] < 10.0, c
                else:                                                    # the unpenalised top is in the halved class and stays the top
                    assert c.halve_class[c.meta["top"]] and before[c.meta["top"]] == 20.0, c
            if c.pen.size >= 8:
                assert {0, V - 1} <= set(c.pen["id"]) and set(c.pen["kind"]) == {0, 1} and set(c.pen["count"]) == {1, 2, 3, 4, 5}, c
                assert ((c.pen["pre"] != 0) & (c.pen["count"] > 0)).sum() == 1, c
                w, ng = c.meta["was_top"], c.meta["negative"]
                assert before[w] == before.max() and after[w] < after[c.meta["top"]], c
                assert before[ng] < 0 and after[ng] > before[ng], c
    g = {c.name: c.expect()[1] for c in cs if c.cls == "G"}
    assert g["inf"]["top_logit"] == np.inf and g["inf"]["ntop"] == 2 and g["inf"]["count"] == 4          # both +inf and both -inf: inf / inf is NaN
    assert 0 < g["subnormal"]["top_logit"] < np.finfo(np.float32).tiny and g["subnormal"]["count"] > 1
    assert g["fltmax"]["top_logit"] == sr.FLT_MAX and g["fltmax"]["count"] >= 2


@pytest.mark.parametrize("V", sr.VS)
def test_ratio_cases_tell_the_exact_quotient_from_its_neighbours(V):
    """every class B case plants at least 16 candidates whose membership under the exact f32 quotient differs both from l * f32(1 / top) < cutoff and from the
    quotient and comparison in double; recomputed here from the case's logits, not taken from the generator's word"""
    bs = sr.pick(V, "B")
    assert len(bs) == 6 and sorted(set(float(c.cutoff_of[c.ids[0]]) for c in bs)) == [float(sr.CUT_LO), float(sr.CUT_MID), float(sr.CUT_HI)]
    for c in bs:
        after, e = c.expect()
        top, cut = e["top_logit"], e["cutoff"]
        assert 5 <= top <= 40 and e["top_id"] == c.ids[0]
        planted = after[c.meta["planted"]]
        with np.errstate(all="ignore"):
            exact = ~(planted / np.float32(top) < np.float32(cut))
            recip = ~(planted * np.float32(np.float32(1.0) / np.float32(top)) < np.float32(cut))
            dbl = ~(planted.astype(np.float64) / np.float64(top) < np.float64(cut))
        assert planted.size >= 16 and ((exact != recip) & (exact != dbl)).sum() >= 16, c
        near = np.abs(after[c.ids[1:]].view(np.uint32).astype(np.int64) - int((np.float32(cut) * np.float32(top)).view(np.uint32)))
        assert near.max() <= 3 and set(near) == {0, 1, 2, 3}, c        # everything planted sits within 3 ulp of cutoff * top, every distance taken
        assert np.array_equal(exact, np.isin(c.meta["planted"], e["ids"]))


@pytest.mark.parametrize("V", sr.VS)
def test_penalty_cases_tell_the_arithmetic(V):
    """every class H case with kind-1 / pre entries has at least 8 entries where (float) ((double) l * d) differs from l * (float) d, and every case with
    counts above 1 an entry where the sequence of products differs from one product by the power; recomputed here from the case's list and logits"""
    hs = sr.pick(V, "H")
    assert sorted(set(c.pen.size for c in hs)) == [n for n in (0, 1, 255, 256, 257, 512) if n <= V - 8] and [c.halve for c in hs].count(1) == 3
    for c in hs:
        before = c.logits()
        n_double = n_count = 0
        for e in c.pen:
            l = before[e["id"]]
            if e["pre"] != 0:
                n_double += np.float32(np.float64(l) * e["pre"]) != np.float32(l * np.float32(e["pre"]))
                first = last = None
                if e["kind"] == 0 and e["count"] > 0:                    # ... and the pre has to come before the counts
                    first, last = np.float32(np.float64(l) * e["pre"]), l
                    for _ in range(e["count"]):
                        first, last = np.float32(first * e["f"]), np.float32(last * e["f"])
                    last = np.float32(np.float64(last) * e["pre"])
                assert first is not None and first != last, c
            elif e["kind"] == 1:
                n_double += np.float32(np.float64(l) * e["d"]) != np.float32(l * np.float32(e["d"]))
            elif e["count"] > 1:
                seq = l
                for _ in range(e["count"]):
                    seq = np.float32(seq * e["f"])
                p = np.float64(e["f"]) ** int(e["count"])
                n_count += seq != np.float32(l * np.float32(p)) and seq != np.float32(np.float64(l) * p)
        if ((c.pen["kind"] == 1) | (c.pen["pre"] != 0)).any():
            assert n_double >= 8, (c, n_double)
        if (c.pen["count"][(c.pen["kind"] == 0) & (c.pen["pre"] == 0)] > 1).any():
            assert n_count >= 1, (c, n_count)


def test_penalty_record_is_the_c_struct():
    assert sr.PEN_DTYPE.itemsize == C.sizeof(booster_amd.LogitPenalty) == 32
    for f in ("id", "count", "kind", "f", "d", "pre"):
        assert sr.PEN_DTYPE.fields[f][1] == getattr(booster_amd.LogitPenalty, f).offset == booster_amd.PENALTY_DTYPE.fields[f][1]
    assert C.sizeof(booster_amd.ShortlistHead) == 32 and booster_amd.ShortlistHead.count.offset == 8 and booster_amd.ShortlistHead.cutoff.offset == 28
    assert sr.refused_penalties(300).size == booster_amd.PENALTY_CAP + 1 == sr.PEN_CAP + 1 and booster_amd.SHORTLIST_CAP == sr.CAP
