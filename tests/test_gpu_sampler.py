"""GPU: the sampler prefilter (booster_amd/csrc/bamd_sampler.hip through bamd_logits_shortlist) on its own, against the numpy restatement of the
reference's rule (tests/sampler_ref.py, itself held to the genuine sampler's fixtures in tests/test_sampler_ref.py).  Every case uploads its tables and
logits, runs the prefilter on the context's stream and compares, bit for bit or exactly: every logit read back, every head field, and the returned
(id, value) pairs as a set.  Where the rule's full sort applies (classes A, B, C up to the cap, H) the id set must also be the one of the library's
full-sort path on the host.

One tiny model per vocabulary size; all five sizes of the list load as they are (300, 1024, 1025, 4100, 128256).  The subnormal case of class G (a
subnormal top above subnormal logits) passes as it stands: the kernels' float division keeps subnormals, as the CPU's does."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import sampler_ref as sr
from booster_amd import gguf

pytestmark = pytest.mark.gpu

U32 = np.uint32
A_PARTS = 4                                      # class A at the Llama-3 size has 4008 top positions: four tests of about a thousand calls


@pytest.fixture(scope="module")
def contexts(bamd, tmp_path_factory):
    """V -> a context of 64 positions on a one-layer model of that vocabulary size, built on first use"""
    made = {}
    d = tmp_path_factory.mktemp("sampler")

    def get(V):
        if V not in made:
            p = str(d / ("v%d.gguf" % V))
            gguf.write_synthetic_llama(p, E=256, H=2, Hkv=1, L=1, F=256, V=V, seed=11)
            m = bamd.Model(p)
            made[V] = (m, bamd.Context(m, 64))
        return made[V][1]
    yield get
    for m, ctx in made.values():
        ctx.close(); m.close()


@pytest.fixture(scope="module")
def full_sort(bamd):
    L = bamd.lib()
    L.bamd_janus_shortlist_test.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_int]

    def ids_of(logits, cutoff):
        lg = np.ascontiguousarray(logits, np.float32)
        ids = np.zeros(lg.size, np.int32)
        n = L.bamd_janus_shortlist_test(lg.ctypes.data_as(C.c_void_p), lg.size, float(cutoff), 0, ids.ctypes.data_as(C.c_void_p), lg.size)
        return np.sort(ids[:n])
    return ids_of


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(U32), np.asarray(b, np.float32).view(U32))


def check(bamd, what, after, e, head, ids, vals, got):
    """device result against the restatement's (after, e): logits, head, pairs"""
    bad = np.nonzero(got.view(U32) != after.view(U32))[0]
    assert bad.size == 0, "%s: %d logits differ after the call, first ids %s: device %s, expected %s" % (what, bad.size, bad[:6], got[bad[:6]], after[bad[:6]])
    assert (head["nan"], head["count"], head["ntop"]) == (e["nan"], e["count"], e["ntop"]), "%s: head %s, expected %s" % (what, head, e)
    if e["top_any_of"] is not None:                                      # a top of zero held with both signs: any of them, consistently
        assert head["top_id"] in e["top_any_of"] and head["top_logit"] == e["top_logit"] and after[head["top_id"]] == head["top_logit"], (what, head)
        assert same_bits(head["cutoff"], e["cutoff_of"][head["top_id"]]), (what, head)
    elif e["top_id"] < 0:
        assert head["top_id"] == -1, (what, head)
    else:
        assert head["top_id"] == e["top_id"] and same_bits(head["top_logit"], e["top_logit"]) and same_bits(head["cutoff"], e["cutoff"]), \
            "%s: head %s, expected %s" % (what, head, {k: e[k] for k in ("top_id", "top_logit", "cutoff")})
        assert same_bits(after[head["top_id"]], head["top_logit"]), what
    n = min(e["count"], bamd.SHORTLIST_CAP)
    gi, gv = ids[:n], vals[:n]
    assert np.unique(gi).size == n and (n == 0 or (gi.min() >= 0 and gi.max() < after.size)), "%s: duplicate or stray ids" % what
    assert same_bits(gv, after[gi]), "%s: a returned value is not the logit of its id" % what
    if e["count"] <= bamd.SHORTLIST_CAP:
        assert np.array_equal(np.sort(gi), e["ids"]), "%s: candidates missing %s, extra %s" % (what, np.setdiff1d(e["ids"], gi)[:8], np.setdiff1d(gi, e["ids"])[:8])
    else:
        assert np.isin(gi, e["ids"]).all(), "%s: a returned id is no candidate" % what
    assert (ids[n:] == bamd.SHORTLIST_SENTINEL_ID).all() and (vals[n:].view(U32) == bamd.SHORTLIST_SENTINEL_BITS).all(), "%s: written past the count / the cap" % what


def run_case(bamd, ctx, c):
    """the procedure of every case; returns (after, e, device ids sorted)"""
    after, e = c.expect()
    e["cutoff_of"] = c.cutoff_of
    ctx.sampler_tables(c.halve_class, c.cutoff_of)
    ctx.set_logits(c.logits())
    head, ids, vals = ctx.logits_shortlist(c.pen, c.halve)
    got = ctx.last_logits()
    check(bamd, repr(c), after, e, head, ids, vals, got)
    return after, e, np.sort(ids[:min(head["count"], bamd.SHORTLIST_CAP)])


def witnessed(c, e):
    return c.cls in "ABH" or (c.cls == "C" and e["count"] <= sr.CAP)


def class_params():
    out = []
    for V in sr.VS:
        for k in "ABCDEFGH":
            if k == "C" and V < 4100:
                continue
            parts = A_PARTS if (k == "A" and V > 5000) else 1
            out += [pytest.param(k, V, p, parts, id="%s-V%d%s" % (k, V, "-part%d" % p if parts > 1 else "")) for p in range(parts)]
    return out


@pytest.mark.parametrize("klass,V,part,parts", class_params())
def test_class(bamd, contexts, full_sort, klass, V, part, parts):
    """every case of a class (tests/sampler_ref.py: A plain, B ratio-test boundary, C cap, D ties, E top <= 0, F NaN, G infinities / subnormals / FLT_MAX,
    H penalties) at one vocabulary size, and the second witness where it applies"""
    ctx = contexts(V)
    cs = sr.pick(V, klass)[part::parts]
    assert cs
    with ThreadPoolExecutor(max_workers=8) as pool:                       # the host's full sorts (ctypes releases the GIL) while the device runs the next cases
        for i in range(0, len(cs), 32):
            jobs = []
            for c in cs[i:i + 32]:
                after, e, dev_ids = run_case(bamd, ctx, c)
                if witnessed(c, e):
                    assert e["nan"] == 0 and e["ntop"] == 1 and e["top_logit"] > 0, c
                    jobs.append((c, dev_ids, pool.submit(full_sort, after, e["cutoff"])))
            for c, dev_ids, f in jobs:
                assert np.array_equal(dev_ids, f.result()), "%r: the device's id set is not the full sort's" % c


@pytest.mark.parametrize("V", [1025, 128256])
def test_too_many_penalties_are_refused(bamd, contexts, V):
    """BAMD_PENALTY_CAP + 1 entries: an error, and the device logits are what they were"""
    ctx = contexts(V)
    c = sr.pick(V, "A")[0]
    ctx.sampler_tables(c.halve_class, c.cutoff_of)
    x = c.logits()
    ctx.set_logits(x)
    with pytest.raises(bamd.BamdError):
        ctx.logits_shortlist(sr.refused_penalties(V), 0)
    assert same_bits(ctx.last_logits(), x)
    run_case(bamd, ctx, c)                                                # and the context still works


@pytest.mark.parametrize("V", [4100, 128256])
def test_no_state_survives_a_call(bamd, contexts, V):
    """one context: several NaNs, a three-way tie, 3000 candidates, then a plain case — its head shows nan 0, ntop 1 and its own count"""
    ctx = contexts(V)
    for c in (sr.pick(V, "F", "several")[0], sr.pick(V, "D", "ties3")[0], sr.pick(V, "C", "n3000")[0]):
        run_case(bamd, ctx, c)
    c = sr.pick(V, "A")[3]
    ctx.sampler_tables(c.halve_class, c.cutoff_of)
    ctx.set_logits(c.logits())
    head, ids, vals = ctx.logits_shortlist(c.pen, c.halve)
    e = c.expect()[1]
    assert (head["nan"], head["ntop"], head["count"]) == (0, 1, e["count"]) and 1 < e["count"] < 10
    assert (ids[e["count"]:] == bamd.SHORTLIST_SENTINEL_ID).all()
    run_case(bamd, ctx, c)


def test_refused_without_tables(bamd, contexts):
    """a context that never had bamd_sampler_tables refuses the call"""
    contexts(300)
    ctx = bamd.Context(contexts(300).model, 64)
    try:
        ctx.set_logits(sr.pick(300, "A")[0].logits())
        with pytest.raises(bamd.BamdError):
            ctx.logits_shortlist(np.zeros(0, sr.PEN_DTYPE), 0)
    finally:
        ctx.close()


@pytest.mark.parametrize("readback", [True, False])
@pytest.mark.parametrize("V", sr.VS)
def test_after_a_real_evaluation(bamd, contexts, V, readback):
    """the prefilter on the logits an evaluation left on the device, with a penalty on the arg-max token: the host mirror follows (bamd_get_logits returns the
    penalised logits), head and set are the restatement's of the lm_head's logits; with the per-decode read-back on and off"""
    ctx = contexts(V)
    cls, cut, _ = sr.tables(V)
    ctx.sampler_tables(cls, cut)
    ctx.set_logits_readback(readback)
    try:
        lg = ctx.decode([1 + int(readback)], 0)
        assert np.isfinite(lg).all() and lg.max() > 0
        t = int(np.argmax(lg))
        pen = np.zeros(1, sr.PEN_DTYPE); pen[0] = (t, 2, 0, np.float32(0.75), 1.0, sr.janus_pre(3, 100))
        head, ids, vals = ctx.logits_shortlist(pen, 1)
        got = ctx.last_logits()
    finally:
        ctx.set_logits_readback(True)
    after = sr.apply_penalties(lg, pen, cls, 1)
    e = sr.shortlist(after, cut); e["cutoff_of"] = cut
    assert after[t] != lg[t] and not same_bits(after, lg)
    check(bamd, "after decode, V=%d readback=%s" % (V, readback), after, e, head, ids, vals, got)
