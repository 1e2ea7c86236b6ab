"""CPU: the whole-model harness itself (tests/refmodel.py).  Every committed reference fixture loads through its family and agrees with its generator's CONFIGS
entry; and check_step, which decides whether an implementation is bit-exact against the reference, still fails on each kind of single-bit difference."""
import numpy as np
import pytest

import refmodel
import test_gpu_float_ref
import test_gpu_iq4nl_ref
import test_gpu_legacy1_ref
import test_gpu_legacy_ref
import test_gpu_lowbit_ref
from refmodel import FLOAT, FULLSIZE, IQ4NL, LEGACY, LEGACY1, LOWBIT, check_step, digest, load_fixture

# the cfgs each family's test file parametrises (tests/test_gpu_fullsize_ref.py names every entry of its generator in a test of its own)
CFGS = [(FULLSIZE, c) for c in FULLSIZE.gen.CONFIGS] + [(LOWBIT, c) for c in test_gpu_lowbit_ref.ALL] + [(LEGACY, c) for c in test_gpu_legacy_ref.ALL] + \
       [(LEGACY1, c) for c in test_gpu_legacy1_ref.ALL] + [(FLOAT, c) for c in test_gpu_float_ref.ALL] + [(IQ4NL, c) for c in test_gpu_iq4nl_ref.ALL]
# where the three counts stand in a CONFIGS entry of 4 (fullsize), 5 (a recipe behind the model) and 6 fields (recipe kwargs and `tied` behind the model)
COUNTS_AT = {4: 1, 5: 2, 6: 3}


def test_the_six_families():
    assert [f.name for f in refmodel.FAMILIES] == ["fullsize", "lowbit", "legacy", "legacy1", "float", "iq4nl"]
    assert [f.prefix for f in refmodel.FAMILIES] == ["fullsize_", "lowbit_", "legacy_", "legacy1_", "float_", ""]


@pytest.mark.parametrize("fam,cfg", CFGS, ids=["%s-%s" % (f.name, c) for f, c in CFGS])
def test_fixture_loads_and_agrees_with_its_generator(fam, cfg):
    entry = fam.gen.CONFIGS[cfg]
    at = COUNTS_AT[len(entry)]
    kw, n_prompt, n_decode, n_ctx = fam.shape(cfg)
    assert kw is entry[0] and (n_prompt, n_decode, n_ctx) == tuple(entry[at:at + 3]) and at + 3 == len(entry)
    assert all(isinstance(v, int) for v in (n_prompt, n_decode, n_ctx)) and 0 < n_prompt < n_ctx
    fx = load_fixture(fam, cfg)
    assert len(fx["tokens"]) == n_decode + 1
    assert fx["probes"].shape == (n_decode + 1, fx["pidx"].size) and fx["top"].shape[0] == n_decode + 1 and fx["digest"].size == n_decode + 1
    assert np.isfinite(fx["probes"]).all() and np.isfinite(fx["top"]).all()


V, N_PROBES = 512, 32


def synthetic():
    """a random logits vector with a -0.0 in it, and the one-step fixture the reference would have recorded for it"""
    rng = np.random.default_rng(20)
    logits = rng.standard_normal(V).astype(np.float32)
    pidx = np.sort(rng.choice(V, N_PROBES, replace=False)).astype(np.int32)
    top = int(np.argmax(logits))
    free = [i for i in range(V) if i not in set(pidx.tolist()) and i != top]         # indices that only the digest sees
    logits[free[0]] = np.float32(-0.0)
    fx = dict(tokens=np.array([top], np.int32), digest=np.array([digest(logits)], "<u8"), pidx=pidx, probes=logits[pidx][None, :].copy(),
              top=np.array([logits.max()], np.float32))
    return logits, fx, free


def flip_lowest_mantissa_bit(logits, i):
    out = logits.copy()
    out.view(np.uint32)[i] ^= 1
    return out


def test_check_step_passes_on_the_recorded_vector():
    logits, fx, _ = synthetic()
    check_step(fx, 0, logits, "self")


def test_check_step_sees_one_bit_at_a_probe():
    logits, fx, _ = synthetic()
    i = int(fx["pidx"][5]) if int(fx["pidx"][5]) != int(fx["tokens"][0]) else int(fx["pidx"][6])
    with pytest.raises(AssertionError, match="probe logits"):
        check_step(fx, 0, flip_lowest_mantissa_bit(logits, i), "probe")


def test_check_step_sees_one_bit_that_only_the_digest_covers():
    logits, fx, free = synthetic()
    with pytest.raises(AssertionError, match="digest"):
        check_step(fx, 0, flip_lowest_mantissa_bit(logits, free[1]), "digest")


def test_check_step_sees_the_maximum_move():
    logits, fx, free = synthetic()
    moved = logits.copy()
    moved[free[2]] = np.float32(logits.max() * 2)
    with pytest.raises(AssertionError, match="arg-max token"):
        check_step(fx, 0, moved, "arg-max")


def test_check_step_tells_minus_zero_from_zero():
    logits, fx, free = synthetic()
    assert logits[free[0]] == 0 and np.signbit(logits[free[0]])
    swapped = logits.copy()
    swapped[free[0]] = np.float32(0.0)
    assert np.array_equal(swapped, logits)                                            # equal as numbers: only a comparison of the bits tells them apart
    with pytest.raises(AssertionError, match="digest"):
        check_step(fx, 0, swapped, "-0.0")
