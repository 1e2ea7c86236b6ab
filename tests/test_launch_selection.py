"""CPU: which kernel instance, grid, LDS size and argument block the mat-vec launchers pick for the launch shapes of the supported models.

A shape that falls off its fast instance lands on the generic kernel and computes the same bits, so no GPU test notices; this pins the selection itself.
booster_amd.trace_matvec / trace_attn_wo ask the launchers through their recording path (host code only: nothing is launched), and every answer is
compared with tests/golden/launch_selection.json.  The golden was recorded from the launchers BEFORE their dispatch code was consolidated and is the
reference for them; when a kernel change moves a launch on purpose, regenerate it (python tests/test_launch_selection.py --regen), review the diff of
the golden and say why in the commit.

The switches (BAMD_* environment variables) are read once per process, so each non-default setting runs the cases it can affect in a fresh child.
"""
import itertools
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_selection.json")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)                 # also run as a script (the children of test_switch_selection, --regen)

Q2_K, Q3_K, Q4_K, Q5_K, Q6_K = 10, 11, 12, 13, 14
TYPES = (Q4_K, Q5_K, Q6_K, Q3_K, Q2_K)
PLAIN, NORM = 0, 1
STORE, ADD, SILU_MUL, ARGMAX = 0, 1, 2, 3
N_CU = (256, 240, 64)            # 256: the MI355X; the others leave a remainder of row-groups and make the grid clamp bite
MODES = (0, 1, 2, 16, 17, 18)
#          E      F     KV rows  V
MODELS = {
    "llama3-8b":   (4096, 14336, 1024, 128256),
    "mistral-7b":  (4096, 14336, 1024, 32000),
    "llama3-70b":  (8192, 28672, 1024, 128256),
    "llama2-7b":   (4096, 11008, 4096, 32000),
    "llama2-13b":  (5120, 13824, 5120, 32000),
    "llama3.2-3b": (3072, 8192, 1024, 128256),
}


def _launches():
    """the mat-vec launches of a decode layer + lm_head, as (kind, K, pro, epi, [(type, rows), ...]); segments as qkv_segments / seg_of build them"""
    out = []
    def add(kind, k, pro, epi, segs):
        c = (kind, k, pro, epi, tuple(segs))
        if c not in out:
            out.append(c)
    for E, F, KV, V in MODELS.values():
        for t in TYPES:
            add("qkv", E, NORM, STORE, [(t, E + 2 * KV)])
            add("wo", E, PLAIN, ADD, [(t, E)])
            add("gateup", E, NORM, SILU_MUL, [(t, F), (t, F)])
            add("down", F, PLAIN, ADD, [(t, E)])
            add("lm_head", E, NORM, ARGMAX, [(t, V)])
        for ta, tb in itertools.permutations(TYPES, 2):                  # wq | wk of one type, wv of another
            add("qkv", E, NORM, STORE, [(ta, E + KV), (tb, KV)])
        add("qkv", E, NORM, STORE, [(Q4_K, E), (Q5_K, KV), (Q6_K, KV)])
    for t in TYPES:                                                      # ragged row counts: padded to 8 in the stream, nvalid = the real rows
        add("wo", 4096, PLAIN, ADD, [(t, 4090)])
        add("down", 14336, PLAIN, ADD, [(t, 4090)])
        add("qkv", 4096, NORM, STORE, [(t, 6139)])
        add("gateup", 4096, NORM, SILU_MUL, [(t, 14331), (t, 14331)])
        add("lm_head", 4096, NORM, ARGMAX, [(t, 32001)])
    add("qkv", 4096, NORM, STORE, [(Q4_K, 5117), (Q6_K, 1021)])
    add("qkv", 4096, NORM, STORE, [(1, 6144)])                           # f16: no kernel, refused
    add("wo", 4096, PLAIN, ADD, [(8, 4096)])                             # q8_0: no kernel, refused
    return out


def _colaunches():
    """(H, Hkv, hd, n_ctx, lds_ld, with_cellpos, wo type, wo rows, K, n_cu)"""
    out = []
    for K in (4096, 8192):
        for hd in (64, 128, 192, 256):
            H = K // hd if K % hd == 0 else (24 if K == 4096 else 48)    # hd 192 divides neither width: the launcher never relates K to H * hd
            for gq in (1, 4, 8):
                for t in TYPES:
                    for n_cu in N_CU:
                        out.append((H, H // gq, hd, 2048, 512, 0, t, K, K, n_cu))
    out.append((32, 8, 128, 2048, 512, 1, Q4_K, 4096, 4096, 256))       # must decline: cell positions tracked
    out.append((32, 8, 128, 2048, 512, 0, Q4_K, 4096, 4096, 36))        # must decline: fewer than 8 wo workgroups
    out.append((24, 8, 128, 2048, 512, 0, Q4_K, 3072, 3072, 256))       # must decline: K = 3072
    out.append((32, 8, 128, 2048, 512, 0, Q6_K, 4090, 4096, 256))       # ragged wo rows
    out.append((32, 8, 128, 256, 0, 0, Q4_K, 4096, 4096, 256))          # lds_ld 0: the padded n_ctx
    out.append((32, 8, 128, 32768, 32768, 0, Q4_K, 4096, 4096, 256))    # must decline: score rows beyond the LDS
    return out


MUST_DECLINE = [c for c in _colaunches() if c[5] or c[9] - c[0] < 8 or c[8] == 3072 or c[4] == 32768]


def _key(kind, k, pro, epi, segs):
    return "%s K%d p%de%d %s" % (kind, k, pro, epi, "|".join("%d:%d" % s for s in segs))


# switch setting -> (cases of the mat-vec list it can affect, modes, whether the co-launch list runs).  Modes >= 16 force the generic kernels: no switch moves them
def _nseg2(c): return c[0] == "qkv" and len(c[4]) == 2
SWITCHES = {
    "BAMD_MV_GENERIC=1":     (lambda c: True, (0, 1, 2), False),
    "BAMD_MIXED_SPLIT=0":    (_nseg2, (0,), False),
    "BAMD_QKV70_WAVES=8":    (lambda c: _nseg2(c) and c[1] == 8192, (0,), False),
    "BAMD_QKV70_WAVES=16":   (lambda c: _nseg2(c) and c[1] == 8192, (0,), False),
    "BAMD_DOWN14=0":         (lambda c: c[2] == PLAIN and c[1] == 14336, (0, 2), False),
    "BAMD_DOWN112=0":        (lambda c: c[2] == PLAIN and c[1] == 28672, (0, 2), False),
    "BAMD_WO4=0":            (lambda c: c[2] == PLAIN and c[3] == ADD and c[1] == 8192, (0, 2), False),
    "BAMD_QKV3=0":           (lambda c: c[0] == "qkv" and len(c[4]) == 1 and c[1] == 4096, (0,), False),
    "BAMD_GATEUP7=0":        (lambda c: c[0] == "gateup" and c[1] == 4096, (0,), False),
    "BAMD_GATEUP14=0":       (lambda c: c[0] == "gateup" and c[1] == 8192, (0,), False),
    "BAMD_COLAUNCH=0":       (None, (), True),
    "BAMD_COLAUNCH70=1":     (None, (), True),
    "BAMD_COLAUNCH_DELAY=0": (None, (), True),
}


def _walk(setting=None):
    """the section of the golden for one switch setting (None: defaults), computed in THIS process: {"matvec": {key: [record per (n_cu, mode)]}, "colaunch": [...]}
    with record = None (refused / declined) or (kernel name, grid, block, lds, kernarg bytes, kernarg hash)"""
    import booster_amd
    sel, modes, co = (lambda c: True, MODES, True) if setting is None else SWITCHES[setting]
    def rec(r):
        return None if r is None else (r["kernel"], r["grid"], r["block"], r["lds"], r["kernarg_bytes"], "%016x" % r["kernarg_hash"])
    sec = {"matvec": {}, "colaunch": []}
    for c in _launches() if sel else []:
        if sel(c):
            kind, k, pro, epi, segs = c
            sec["matvec"][_key(*c)] = [rec(booster_amd.trace_matvec(segs, k, pro, epi, mode, n_cu)) for n_cu in N_CU for mode in modes]
    if co:
        for H, Hkv, hd, n_ctx, ld, cp, t, rows, k, n_cu in _colaunches():
            sec["colaunch"].append(rec(booster_amd.trace_attn_wo(H, Hkv, hd, n_ctx, ld, t, rows, k, n_cu, il=3, with_cellpos=cp)))
    return sec


# ---- storage: a table of kernel names, a table of distinct (name, grid, block, lds, kernarg bytes), and per case "launch index:kernarg hash" (or null) ----
def _pack(sections):
    names, shapes = [], []
    def idx(tab, v):
        if v not in tab:
            tab.append(v)
        return tab.index(v)
    def enc(r):
        if r is None:
            return None
        name, grid, block, lds, nbytes, h = r
        return "%d:%s" % (idx(shapes, [idx(names, name), list(grid), list(block), lds, nbytes]), h)
    out = {}
    for s, sec in sections.items():
        out[s] = {"matvec": {k: [enc(r) for r in v] for k, v in sec["matvec"].items()}, "colaunch": [enc(r) for r in sec["colaunch"]]}
    return {"kernels": names, "launches": shapes, "sections": out}


def _unpack_section(g, s):
    def dec(e):
        if e is None:
            return None
        i, h = e.split(":")
        n, grid, block, lds, nbytes = g["launches"][int(i)]
        return (g["kernels"][n], grid, block, lds, nbytes, h)
    sec = g["sections"][s]
    return {"matvec": {k: [dec(e) for e in v] for k, v in sec["matvec"].items()}, "colaunch": [dec(e) for e in sec["colaunch"]]}


def _norm(sec):                  # tuples / lists compare equal after a JSON round trip
    return json.loads(json.dumps(sec))


def _child(setting):
    name, val = setting.split("=")
    env = dict(os.environ); env[name] = val
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--walk", setting], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.splitlines()[-1])


def _compare(got, want, what):
    got, want = _norm(got), _norm(want)
    assert list(got["matvec"]) == list(want["matvec"]), "%s: the case list differs from the golden's" % what
    bad = []
    for key in want["matvec"]:
        modes = MODES if what == "default" else SWITCHES[what][1]
        labels = ["n_cu %d mode %d" % (n, m) for n in N_CU for m in modes]
        for lab, g, w in zip(labels, got["matvec"][key], want["matvec"][key]):
            if g != w:
                bad.append("%s [%s]\n    golden %s\n    now    %s" % (key, lab, w, g))
    assert len(got["colaunch"]) == len(want["colaunch"]), "%s: the co-launch case list differs from the golden's" % what
    for c, g, w in zip(_colaunches(), got["colaunch"], want["colaunch"]):
        if g != w:
            bad.append("colaunch %s\n    golden %s\n    now    %s" % (c, w, g))
    assert not bad, "%s: %d launches differ from the golden:\n%s" % (what, len(bad), "\n".join(bad[:20]))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_default_selection(golden):
    got = _walk()
    n = sum(len(v) for v in got["matvec"].values()) + len(got["colaunch"])
    assert n > 4000                                                      # the list is not shortened
    _compare(got, _unpack_section(golden, "default"), "default")


def test_refused_and_declined(golden):
    sec = _unpack_section(golden, "default")
    for key in ("qkv K4096 p1e0 1:6144", "wo K4096 p0e1 8:4096"):
        assert all(r is None for r in sec["matvec"][key])
    cases = _colaunches()
    for c in MUST_DECLINE:
        assert sec["colaunch"][cases.index(c)] is None, c
    assert sum(r is not None for r in sec["colaunch"]) > 100             # and the co-launch does take its shapes


@pytest.mark.parametrize("setting", list(SWITCHES))
def test_switch_selection(golden, setting):
    _compare(_child(setting), _unpack_section(golden, setting), setting)


if __name__ == "__main__":
    if "--walk" in sys.argv:                                             # child of test_switch_selection: one section, computed under this process's environment
        print(json.dumps(_walk(sys.argv[sys.argv.index("--walk") + 1])))
    elif "--regen" in sys.argv:
        sections = {"default": _walk()}
        for s in SWITCHES:
            sections[s] = _child(s)
        g = _pack(sections)
        j = lambda v: json.dumps(v, separators=(",", ":"))
        rows = lambda tab: ",\n".join("  " + j(v) for v in tab)
        with open(GOLDEN, "w") as f:                                     # one line per kernel, per launch and per case list: diffs stay readable
            f.write('{"kernels":[\n%s\n],\n"launches":[\n%s\n],\n"sections":{\n' % (rows(g["kernels"]), rows(g["launches"])))
            secs = []
            for s, sec in g["sections"].items():
                mv = ",\n".join("  %s:%s" % (j(k), j(v)) for k, v in sec["matvec"].items())
                secs.append('%s:{"matvec":{\n%s\n},\n"colaunch":%s}' % (j(s), mv, j(sec["colaunch"])))
            f.write(",\n".join(secs) + "\n}}\n")
        json.load(open(GOLDEN))
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
