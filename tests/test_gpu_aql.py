"""GPU: the own AQL queue (csrc/bamd_aql.h) is the path that RUNS by default — not a silent fall-back to the hipGraph — and gives the hipGraph path's bits:
  * the device-side greedy loop on the genuine reference's tiny fixture (single-launch attention) and on a longer sequence (scores | softmax + P.V);
  * single-token bamd_decode steps (the bridge's token loop: state from the pinned host inbox);
  * more packets than the queue's ring holds (the wrap), many short replays;
  * ONE call that writes several times the ring (the host waits for room, replay after replay), the same call under a stall limit an eighth of its duration,
    single-token steps across the ring, two contexts of different depth taking turns on the queue, a greedy call that crosses 448 positions.
The reference of all of these is the same sequence of calls with set_aql(False): the same kernels, submitted by the HIP runtime with full ordering — a reference
for the submission, not for the kernels (which have their own oracle tests).  aql_stats() proves which path a call took.
BAMD_AQL=0 in the environment (tools/switch_matrix.sh) turns the assertions about which path ran around."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from goldenio import load_bgld
from booster_amd import gguf

pytestmark = pytest.mark.gpu
OWN_QUEUE = os.environ.get("BAMD_AQL", "1") != "0"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def greedy(bamd, path, n_ctx, prompt, n_steps, aql):
    bamd.set_aql(aql)
    try:
        m = bamd.Model(path); ctx = bamd.Context(m, n_ctx)
        for i in range(0, len(prompt), 512):
            ctx.decode(prompt[i:i + 512], i)
        out, _ = ctx.generate_greedy(len(prompt), n_steps)
        lg = ctx.last_logits()
        runs = ctx.aql_runs()
        ctx.close(); m.close()
        return out, lg, runs
    finally:
        bamd.set_aql(True)


def test_greedy_loop_runs_on_the_own_queue_and_matches_the_hipgraph(bamd):
    g = load_bgld(os.path.join(GOLDEN, "tiny_a.bgld"))
    path = os.path.join(GOLDEN, "tiny_a.gguf")
    prompt, toks = [int(t) for t in g["meta/prompt"]], g["greedy/tokens"]
    out1, lg1, runs1 = greedy(bamd, path, 128, prompt, len(toks), True)
    out0, lg0, runs0 = greedy(bamd, path, 128, prompt, len(toks), False)
    assert runs0 == 0
    assert (runs1 >= 1) == OWN_QUEUE, "the greedy loop did not run where it should (BAMD_AQL_VERBOSE=1 says why the own queue is not used)"
    assert np.array_equal(out1, out0) and np.array_equal(out1[:len(toks)], toks)
    assert np.array_equal(bits(lg1), bits(lg0)) and np.array_equal(bits(lg1), bits(g["greedy/logits"][len(toks)]))


def test_long_sequence_path_on_the_own_queue(bamd, tmp_path):
    """beyond 448 positions the attention is scores | softmax + P.V: the step still replays from the own queue (bamd_attention_split_is_ik_clean)"""
    p = str(tmp_path / "aql_long.gguf")
    gguf.write_synthetic_llama(p, E=1024, H=8, Hkv=2, L=3, F=1792, V=1024, seed=23)
    prompt = [(7919 * i + 13) % 1024 for i in range(700)]
    out1, lg1, runs1 = greedy(bamd, p, 1024, prompt, 24, True)
    out0, lg0, runs0 = greedy(bamd, p, 1024, prompt, 24, False)
    assert runs0 == 0 and (runs1 >= 1) == OWN_QUEUE
    assert np.array_equal(out1, out0) and np.array_equal(bits(lg1), bits(lg0))


def test_single_token_decode_steps_on_the_own_queue(bamd):
    """bamd_decode with one token (the bridge's loop): the step's state travels through the pinned host inbox; every step's logits == the hipGraph path's"""
    path = os.path.join(GOLDEN, "tiny_b.gguf")
    prompt = [5, 9, 2, 77, 31, 8, 1, 40]
    res = {}
    for aql in (True, False):
        bamd.set_aql(aql)
        try:
            m = bamd.Model(path); ctx = bamd.Context(m, 128)
            lg = ctx.decode(prompt, 0)
            rows, n_past = [], len(prompt)
            for _ in range(30):
                t = int(np.argmax(lg))
                lg = ctx.decode([t], n_past); n_past += 1
                rows.append(lg)
            res[aql] = (np.array(rows), ctx.aql_runs())
            ctx.close(); m.close()
        finally:
            bamd.set_aql(True)
    assert res[False][1] == 0 and (res[True][1] >= 30) == OWN_QUEUE
    assert np.array_equal(bits(res[True][0]), bits(res[False][0]))


def test_many_replays_across_the_ring_wrap(bamd):
    """the queue's ring holds 16384 packets: 400 greedy calls of 20 steps on the tiny model write ~ 5 x that, one doorbell never spanning the wrap (bamd_aql.cpp)"""
    path = os.path.join(GOLDEN, "tiny_a.gguf")
    m = bamd.Model(path); ctx = bamd.Context(m, 128)
    s0 = bamd.aql_stats()
    first = None
    for i in range(400):
        ctx.decode([1, 2, 3, 4, 5, 6, 7, 8], 0)
        out, _ = ctx.generate_greedy(8, 20)
        if first is None:
            first = out.copy()
        assert np.array_equal(out, first), "replay %d differs" % i
    assert (ctx.aql_runs() >= 400) == OWN_QUEUE
    s1 = bamd.aql_stats()
    if OWN_QUEUE:
        assert s1["packets"] - s0["packets"] > s1["ring"], "the replays did not go round the ring"
        assert s1["wrap_doorbells"] - s0["wrap_doorbells"] >= 1, "no replay rang the extra doorbell at the ring's last slot"
    ctx.close(); m.close()


# ---- back-pressure, the stall limit, interleaved producers ------------------------------------------------------------------------------------------
# Small widths (what is tested is the submission, not a kernel shape); 16 layers, so that a step is some 100 packets and the ring fills after a few hundred steps.
LONG_STEPS = 1536
LONG_PROMPT = [5, 9, 2, 77, 31, 8, 1, 40]
LONG_CTX = 2048
STAT_KEYS = ("packets", "room_waits", "wrap_doorbells")


def synth(dirpath, name, L, seed):
    p = str(dirpath / name)
    gguf.write_synthetic_llama(p, E=512, H=8, Hkv=2, L=L, F=768, V=512, seed=seed, reuse_layers=True)
    return p


def delta(a, b):
    return {k: b[k] - a[k] for k in STAT_KEYS}


def long_run(bamd, path, aql, stall_ms=0):
    """a short prompt, ONE greedy call of LONG_STEPS steps (it crosses 448 positions inside the call, so every step is scores | softmax + P.V), then a one-step call
    with the same launch sequence: the packets it writes are the launches per step"""
    bamd.set_aql(aql); bamd.set_aql_stall_ms(stall_ms)
    try:
        m = bamd.Model(path); ctx = bamd.Context(m, LONG_CTX)
        ctx.decode(LONG_PROMPT, 0)
        s0 = bamd.aql_stats()
        out, ms = ctx.generate_greedy(len(LONG_PROMPT), LONG_STEPS)
        lg = ctx.last_logits()
        s1 = bamd.aql_stats()
        out_one, _ = ctx.generate_greedy(len(LONG_PROMPT) + LONG_STEPS, 1)
        lg_one = ctx.last_logits()
        s2 = bamd.aql_stats()
        r = dict(out=out, lg=lg, ms=ms, out_one=out_one, lg_one=lg_one, runs=ctx.aql_runs(), long=delta(s0, s1), lps=s2["packets"] - s1["packets"], ring=s2["ring"])
        ctx.close(); m.close()
        return r
    finally:
        bamd.set_aql(True); bamd.set_aql_stall_ms(0)


def same_bits(a, b):
    return (np.array_equal(a["out"], b["out"]) and np.array_equal(bits(a["lg"]), bits(b["lg"])) and
            np.array_equal(a["out_one"], b["out_one"]) and np.array_equal(bits(a["lg_one"]), bits(b["lg_one"])))


@pytest.fixture(scope="module")
def long_model(tmp_path_factory):
    return synth(tmp_path_factory.mktemp("aql_long16"), "aql_l16.gguf", 16, 29)


@pytest.fixture(scope="module")
def long_ref(bamd, long_model):
    """the hipGraph run of long_run's calls: computed once, compared against, never changed"""
    r = long_run(bamd, long_model, False)
    assert r["runs"] == 0 and r["long"] == dict.fromkeys(STAT_KEYS, 0) and r["lps"] == 0
    return r


def test_one_run_longer_than_the_ring(bamd, long_model, long_ref):
    """one bamd_aql_run call writes >= 2.5 x the ring: the host gets ahead of the GPU and waits for room before most replays.  Measured on the MI355X:
    ring 16384, 98 launches per step, 1536 steps = 150 528 packets = 9.2 rings, room_waits + 1369 of 1536 replays."""
    own = long_run(bamd, long_model, True)
    print("ring %d, launches per step %d, steps %d, long call: %s, %.1f ms" % (own["ring"], own["lps"], LONG_STEPS, own["long"], own["ms"]))
    assert (own["runs"] >= 2) == OWN_QUEUE
    if OWN_QUEUE:
        assert own["lps"] > 0 and LONG_STEPS * own["lps"] >= 2.5 * own["ring"], "the call is too short to test back-pressure"
        assert own["long"]["packets"] == LONG_STEPS * own["lps"]
        assert own["long"]["room_waits"] >= 1, "the host never found the ring full: nothing was tested"
    else:
        assert own["long"] == dict.fromkeys(STAT_KEYS, 0) and own["lps"] == 0 and own["ring"] == 0
    assert same_bits(own, long_ref)
    # the hipGraph result itself: a fresh context fed the same tokens one at a time.  The prompt stays the one batch it is in every run here: a prompt evaluated
    # as a batch and the same prompt evaluated token by token are two different computations in the reference too (the oracle gives other bits for each, and this
    # library matches it in both), so only the tokens of the greedy call are fed singly
    bamd.set_aql(False)
    try:
        m = bamd.Model(long_model); ctx = bamd.Context(m, LONG_CTX)
        ctx.decode(LONG_PROMPT, 0)
        for i, t in enumerate(long_ref["out"][:LONG_STEPS]):
            lg = ctx.decode([int(t)], len(LONG_PROMPT) + i)
        assert ctx.aql_runs() == 0
        ctx.close(); m.close()
    finally:
        bamd.set_aql(True)
    assert np.array_equal(bits(lg), bits(long_ref["lg"])) and int(np.argmax(lg)) == int(long_ref["out"][LONG_STEPS])


def test_run_outlasts_the_stall_limit(bamd, long_model, long_ref):
    """the limit bounds a stall of the queue's read index, not the run: the call of the test above, again with a limit of an eighth of its own duration (under the
    former rule, one deadline for the whole call, it fails with "the queue stopped consuming packets").  Measured on the MI355X: T = 641 ms, stall = 80 ms;
    with the former rule built in for once, the second call failed with exactly that text."""
    first = long_run(bamd, long_model, True)
    T = first["ms"]
    stall = max(20, int(T / 8))
    print("T = %.1f ms, stall = %d ms" % (T, stall))
    if OWN_QUEUE:
        assert T >= 160 and T >= 8 * stall, "the call is too short to outlast a stall limit"
    second = long_run(bamd, long_model, True, stall_ms=stall)
    assert (first["runs"] >= 2) == OWN_QUEUE and (second["runs"] >= 2) == OWN_QUEUE
    if OWN_QUEUE:
        assert second["long"]["packets"] == LONG_STEPS * second["lps"] and second["long"]["room_waits"] >= 1
    assert same_bits(first, long_ref) and same_bits(second, long_ref)


def test_single_token_steps_across_the_ring(bamd, tmp_path):
    """the bridge's loop: one bamd_aql_run call per token, until the packets written exceed one ring (two layers: some 1 700 host round trips)"""
    path = synth(tmp_path, "aql_l2.gguf", 2, 31)
    prompt, n_ctx = [3, 1, 4, 1, 5, 9, 2, 6], 3072
    cap = n_ctx - len(prompt) - 1
    res = {}
    for aql in (True, False):
        bamd.set_aql(aql)
        try:
            m = bamd.Model(path); ctx = bamd.Context(m, n_ctx)
            lg = ctx.decode(prompt, 0)
            s0 = bamd.aql_stats()
            rows, fed, n_past = [], [], len(prompt)
            if aql:
                while len(rows) < (cap if OWN_QUEUE else 1700) and bamd.aql_stats()["packets"] - s0["packets"] <= s0["ring"]:
                    fed.append(int(np.argmax(lg)))
                    lg = ctx.decode([fed[-1]], n_past); n_past += 1
                    rows.append(lg)
            else:
                for t in res[True][2]:                                   # the same tokens: a difference shows at the step it arises
                    lg = ctx.decode([t], n_past); n_past += 1
                    rows.append(lg)
            res[aql] = (np.array(rows), ctx.aql_runs(), fed, delta(s0, bamd.aql_stats()))
            ctx.close(); m.close()
        finally:
            bamd.set_aql(True)
    rows1, runs1, fed, d1 = res[True]
    rows0, runs0, _, d0 = res[False]
    print("%d single-token steps, %s" % (len(fed), d1))
    assert runs0 == 0 and d0 == dict.fromkeys(STAT_KEYS, 0)
    assert (runs1 >= len(fed)) == OWN_QUEUE
    if OWN_QUEUE:
        assert d1["packets"] > bamd.aql_stats()["ring"], "the steps did not go round the ring"
    step_differs = np.nonzero((bits(rows1) != bits(rows0)).any(axis=1))[0]
    assert step_differs.size == 0, "first difference at step %d" % step_differs[0]


def test_two_contexts_share_the_queue(bamd, tmp_path):
    """two models of different depth (different launches per step), one context each on the same device, taking turns: the device-wide write index, the wrap and
    the shared completion signal under interleaved producers.  400 calls: greedy calls of 6 steps and of 1 step, single-token steps in between"""
    paths = [synth(tmp_path, "aql_l4.gguf", 4, 37), synth(tmp_path, "aql_l7.gguf", 7, 41)]
    prompts = [[5, 9, 2, 77, 31, 8, 1, 40], [11, 3, 200, 7, 19]]
    res = {}
    for aql in (True, False):
        bamd.set_aql(aql)
        try:
            ms = [bamd.Model(p) for p in paths]; cs = [bamd.Context(m, 1024) for m in ms]
            lgs = [c.decode(pr, 0) for c, pr in zip(cs, prompts)]
            n_past = [len(pr) for pr in prompts]
            s0 = bamd.aql_stats()
            log = ([], [])
            for i in range(400):
                w, kind = i % 2, (i // 2) % 4
                c = cs[w]
                if kind in (0, 2):
                    k = 6 if kind == 0 else 1
                    out, _ = c.generate_greedy(n_past[w], k); n_past[w] += k
                    lgs[w] = c.last_logits()
                    log[w].append(out.astype(np.uint32))
                else:
                    lgs[w] = c.decode([int(np.argmax(lgs[w]))], n_past[w]); n_past[w] += 1
                log[w].append(bits(lgs[w]))
            res[aql] = ([np.concatenate(l) for l in log], [c.aql_runs() for c in cs], delta(s0, bamd.aql_stats()))
            for c in cs: c.close()
            for m in ms: m.close()
        finally:
            bamd.set_aql(True)
    print("two contexts: %s" % res[True][2])
    assert res[False][1] == [0, 0] and res[False][2] == dict.fromkeys(STAT_KEYS, 0)
    assert [r >= 200 for r in res[True][1]] == [OWN_QUEUE, OWN_QUEUE]
    if OWN_QUEUE:
        assert res[True][2]["packets"] > bamd.aql_stats()["ring"], "the calls did not go round the ring"
    for w in (0, 1):
        assert np.array_equal(res[True][0][w], res[False][0][w]), "context %d differs from its hipGraph run" % w


def test_greedy_call_crossing_448_positions(bamd, tmp_path):
    """the replay's key is the attention path of the call's LAST position: a call that begins below the single-launch attention's bound and ends above it runs as
    scores | softmax + P.V from its first step, a call wholly below it as the single launch — on the own queue as on the hipGraph"""
    p = synth(tmp_path, "aql_l3.gguf", 3, 43)
    for n_prompt in (440, 100):
        prompt = [(7919 * i + 13) % 512 for i in range(n_prompt)]
        out1, lg1, runs1 = greedy(bamd, p, 512, prompt, 24, True)
        out0, lg0, runs0 = greedy(bamd, p, 512, prompt, 24, False)
        assert runs0 == 0 and (runs1 >= 1) == OWN_QUEUE, n_prompt
        assert np.array_equal(out1, out0) and np.array_equal(bits(lg1), bits(lg0)), n_prompt
