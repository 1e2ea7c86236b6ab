"""What the tests of the matrix-core prompt kernels (tests/test_gpu_*_mfma.py) share: the family switches, the launch counters and the whole-model runners.
A plain helper module (as goldenio.py); the per-kernel shape tests stay in their files."""
import contextlib
import os

import numpy as np

import refmodel

# what the library read from the environment when it was loaded: the suite is also run under BAMD_PREFILL_Q0=1 / BAMD_PREFILL_Q1=1 / BAMD_PREFILL_NL=1, and the
# tests behind a switched block must still find those settings
ENV = {k: os.environ.get("BAMD_PREFILL_" + k.upper(), "")[:1] == "1" for k in ("lowbit", "q0", "q1", "nl", "flt")}


@contextlib.contextmanager
def prefill_switches(bamd, **on):
    """sets the named family switches (lowbit, q0, q1, nl, flt) through their setters; on exit exactly those go back to the process's defaults"""
    for k, v in on.items():
        getattr(bamd, "set_prefill_" + k)(v)
    try:
        yield
    finally:
        for k in on:
            getattr(bamd, "set_prefill_" + k)(ENV[k])


def runs(bamd, types):
    return {t: bamd.prefill_mfma_runs(t) for t in types}


def layer_types(path, types):
    """the types among `types` that the file's layer matrices have"""
    from booster_amd.gguf import GGUFReader
    r = GGUFReader(path)
    return {int(ti["type"]) for name, ti in r.tensors.items()
            if name.startswith("blk.") and name.endswith(".weight") and len(ti["shape"]) == 2 and int(ti["type"]) in types}


def prompt_step(bamd, path, capfd, types, on, fam=None, cfg=None, fx=None, n_prompt=None, n_ctx=None):
    """loads the file under the switches `on`; returns (load-time stderr, side-table bytes, counters before, counters after) of its prompt step, whose logits it
    checks against the fixture where there is one (cfg of fam gives the prompt length and n_ctx then)"""
    if cfg is not None:
        _, n_prompt, _, n_ctx = fam.shape(cfg)
    capfd.readouterr()
    with prefill_switches(bamd, **on):
        m = bamd.Model(path)
        err = capfd.readouterr().err
        try:
            aux = m.prefill_aux_bytes()
            ctx = bamd.Context(m, n_ctx)
            before = runs(bamd, types)
            logits = ctx.decode(refmodel.prompt_of(n_prompt, m.n_vocab), 0)
            after = runs(bamd, types)
            if fx is not None:
                refmodel.check_step(fx, 0, logits, "%s prompt, switches %r" % (cfg, on))
            else:
                assert np.isfinite(logits).all()
            ctx.close()
        finally:
            m.close()
    return err, aux, before, after


def no_tables_with_the_switches_off(bamd, path, *names):
    with prefill_switches(bamd, **{k: False for k in names}):      # the switches off again: a fresh model of the same file builds no tables
        m = bamd.Model(path)
        try:
            assert m.prefill_aux_bytes() == 0
        finally:
            m.close()


def two_stages_on_the_matrix_cores(bamd, fam, cfg, types, moved, on):
    """cfg's prompt through two layer-split stages (bamd_stage_prefill), cut behind layer 2, under the switches `on`: the counters of the types `moved` move"""
    L = fam.shape(cfg)[0]["L"]
    with prefill_switches(bamd, **on):
        before = runs(bamd, types)
        refmodel.run_config_through_stages(bamd, fam, cfg, [(0, 2), (2, L)], 0)
        after = runs(bamd, types)
    for t in moved:
        assert after[t] > before[t], "no matrix-core launch of type %d: %r -> %r" % (t, before, after)
