"""CPU: the BF16 switch of the prompt matrix-core families (booster_amd/csrc/bamd_prefill_family.h, row BF16; set_prefill_bf16 / BAMD_PREFILL_BF16) beside the
five that tests/test_prefill_family.py walks.  With it on, a BF16 matrix needs no table under every setting of the others and every other type answers as
tests/golden/prefill_reasons.json records; with it off, all 448 answers are the golden's.  The environment variable is read once per process, so its parsing is
checked in fresh children (the --answers mode of tests/test_prefill_family.py)."""
import os

import pytest

import test_prefill_family as pf
from test_prefill_family import golden  # noqa: F401  (fixture)


def _walk(bf16):
    import booster_amd
    booster_amd.set_prefill_bf16(bf16)
    try:
        return pf._walk()
    finally:
        booster_amd.set_prefill_bf16(os.environ.get("BAMD_PREFILL_BF16", "")[:1] == "1")


def test_on_bf16_needs_no_table_and_nothing_else_moves(golden):
    got = _walk(True)
    assert list(got) == list(golden)
    for k in golden:
        assert got[k]["BF16"] == "no table needed", k
        assert {n: a for n, a in got[k].items() if n != "BF16"} == {n: a for n, a in golden[k].items() if n != "BF16"}, k


def test_off_every_answer_is_the_goldens(golden):
    assert _walk(False) == golden


def test_env_one_switches_it_on(golden):
    got = pf._child({"BAMD_PREFILL_BF16": "1"})
    assert got["BF16"] == "no table needed"
    assert {n: a for n, a in got.items() if n != "BF16"} == {n: a for n, a in golden[pf._key(0)].items() if n != "BF16"}
    both = pf._child({"BAMD_PREFILL_BF16": "1", "BAMD_PREFILL_FLT": "1"})      # independent of FLT
    assert both["BF16"] == "no table needed" and both["F16"] == "no table needed"
    assert pf._child({"BAMD_PREFILL_FLT": "1"})["BF16"] == golden[pf._key(16)]["BF16"] != "no table needed"


@pytest.mark.parametrize("value", ["0", "", "yes"])
def test_env_other_values_leave_it_off(golden, value):
    assert pf._child({"BAMD_PREFILL_BF16": value}) == golden[pf._key(0)]
