"""CPU: what a model's side-table build decides for a matrix of every weight type under every setting of the five prompt matrix-core switches
(booster_amd/csrc/bamd_prefill_family.h): "tables", "no table needed" (F32 / F16 with BAMD_PREFILL_FLT on) or the sentence of the load-time message.

The test-only export bamd_prefill_reason_test answers for one type under the current switches (host code only: no device is touched).  The 14 record
types x 32 settings are compared, string for string, with tests/golden/prefill_reasons.json, which was recorded from the commit BEFORE the families were
described in one table (tests/golden/prefill_reasons.txt says how); the sentences are part of the behaviour, so a change of one is a change of the golden that
the commit explains (python tests/test_prefill_family.py --regen).

The environment variables are read once per process, so their parsing is checked in fresh children.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "prefill_reasons.json")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)                 # also run as a script (the children, --regen)

TYPES = {"F32": 0, "F16": 1, "BF16": 30, "Q4_0": 2, "Q4_1": 3, "Q5_0": 6, "Q5_1": 7, "Q8_0": 8, "Q2_K": 10, "Q3_K": 11, "Q4_K": 12, "Q5_K": 13, "Q6_K": 14, "IQ4_NL": 20}
SWITCHES = ("lowbit", "q0", "q1", "nl", "flt")                          # set_prefill_<name>, BAMD_PREFILL_<NAME>; bit i of a setting = switch i
FAMILY = {"lowbit": {"Q2_K", "Q3_K"}, "q0": {"Q4_0", "Q5_0", "Q8_0"}, "q1": {"Q4_1", "Q5_1"}, "nl": {"IQ4_NL"}, "flt": {"F32", "F16"}}
ALWAYS = {"Q4_K", "Q5_K", "Q6_K"}


def _key(setting):
    return " ".join("%s=%d" % (s, setting >> i & 1) for i, s in enumerate(SWITCHES))


def _answers():
    """{type name: answer} under the switches of THIS process as they are now"""
    import booster_amd
    f = booster_amd.lib().bamd_prefill_reason_test
    f.argtypes = [C.c_int]; f.restype = C.c_char_p
    return {n: f(t).decode() for n, t in TYPES.items()}


def _walk():
    """every setting through the public setters; the process's defaults (everything off unless its environment says otherwise) are put back"""
    import booster_amd
    out = {}
    try:
        for setting in range(32):
            for i, s in enumerate(SWITCHES):
                getattr(booster_amd, "set_prefill_" + s)(bool(setting >> i & 1))
            out[_key(setting)] = _answers()
    finally:
        for s in SWITCHES:
            getattr(booster_amd, "set_prefill_" + s)(os.environ.get("BAMD_PREFILL_" + s.upper(), "")[:1] == "1")
    return out


def _child(env_add):
    env = {k: v for k, v in os.environ.items() if not k.startswith("BAMD_PREFILL_")}
    env.update(env_add)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--answers"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.splitlines()[-1])


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    return {k: {n: g["strings"][i] for n, i in zip(g["types"], row)} for k, row in g["cases"].items()}


def test_reason_matrix(golden):
    assert list(golden) == [_key(s) for s in range(32)] and all(list(v) == list(TYPES) for v in golden.values())      # 448 cases, none dropped
    got = _walk()
    bad = ["%s  %s\n    golden %s\n    now    %s" % (k, n, golden[k][n], got[k][n]) for k in golden for n in TYPES if got[k][n] != golden[k][n]]
    assert not bad, "%d of 448 answers differ from the golden:\n%s" % (len(bad), "\n".join(bad[:10]))


def test_golden_is_consistent(golden):
    """the recorded matrix itself: a type has tables (or needs none) exactly while its family's switch is on, whatever the other switches say"""
    for setting in range(32):
        row = golden[_key(setting)]
        on = set(ALWAYS)
        for i, s in enumerate(SWITCHES):
            if setting >> i & 1:
                on |= FAMILY[s]
        assert {n for n in TYPES if row[n] in ("tables", "no table needed")} == on, _key(setting)
        assert {n for n in TYPES if row[n] == "no table needed"} == (FAMILY["flt"] if setting >> 4 & 1 else set())


@pytest.mark.parametrize("switch", SWITCHES)
def test_env_one_switches_on_its_family_only(golden, switch):
    got = _child({"BAMD_PREFILL_" + switch.upper(): "1"})
    assert got == golden[_key(1 << SWITCHES.index(switch))]
    assert {n for n in TYPES if got[n] != golden[_key(0)][n]} >= FAMILY[switch]
    assert {n for n in TYPES if got[n] in ("tables", "no table needed")} == ALWAYS | FAMILY[switch]


@pytest.mark.parametrize("value", ["0", "", "yes"])
def test_env_other_values_leave_every_family_off(golden, value):
    assert _child({"BAMD_PREFILL_" + s.upper(): value for s in SWITCHES}) == golden[_key(0)]


if __name__ == "__main__":
    if "--answers" in sys.argv:                                          # a child: the answers under this process's environment, no setter called
        print(json.dumps(_answers()))
    elif "--regen" in sys.argv:
        got, strings = _walk(), []
        for row in got.values():
            for a in row.values():
                if a not in strings:
                    strings.append(a)
        with open(GOLDEN, "w") as f:                                     # one line per sentence and per setting: diffs stay readable
            f.write('{"types":%s,\n"strings":[\n%s\n],\n"cases":{\n%s\n}}\n' % (
                json.dumps(list(TYPES)), ",\n".join("  " + json.dumps(s) for s in strings),
                ",\n".join("  %s:%s" % (json.dumps(k), json.dumps([strings.index(a) for a in row.values()], separators=(",", ":"))) for k, row in got.items())))
        json.load(open(GOLDEN))
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes,", len(strings), "distinct answers")
