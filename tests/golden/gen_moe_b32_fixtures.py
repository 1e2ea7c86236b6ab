#!/usr/bin/env python3
"""Fixtures of mixture-of-experts models with 32-weight-block experts, from the GENUINE reference (build container only; needs oracle/_ref/ref_run:
`make -C oracle refrun`).  As tests/golden/gen_moe_fixtures.py, whose TINY shape, side-file format and main loop this generator shares, with its own CONFIGS: the
8-expert recipes of booster_amd.gguf.mixtral_b32_type.  Committed: DATA ONLY (tests/golden/moe_b32_<cfg>.bgld, a few KB).

    python tests/golden/gen_moe_b32_fixtures.py [cfg ...]
"""
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from booster_amd import gguf  # noqa: E402

_spec = importlib.util.spec_from_file_location("gen_moe_fixtures", os.path.join(HERE, "gen_moe_fixtures.py"))
moe = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(moe)

TINY = moe.TINY
EIGHT = dict(n_expert=8, n_expert_used=2)
CONFIGS = {
    # name: (model kwargs, expert kwargs, dense recipe of the ftype, n_prompt, n_decode, n_ctx)
    # Q4_0 | Q8_0 | Q8_0 QKV in one launch (one activation form), Q4_0 attn_output and experts, Q6_K output
    "tiny_q4_0": (TINY, EIGHT, gguf.q4_0_type, 24, 24, 64),
    # Q5_1 attn_q (Q8_1 activations) beside Q8_0 attn_k / attn_v: the two-form QKV, two launches per layer; Q5_1 experts: the summs chain in every routed launch
    "tiny_q5_1": (TINY, EIGHT, gguf.q5_1_type, 24, 24, 64),
    # IQ4_NL | Q8_0 | Q8_0 QKV, Q5_K attn_output, IQ4_NL gate / up experts, Q5_K down experts in the first layer (L / 8 = 1) and IQ4_NL ones behind it
    "tiny_iq4nl": (TINY, EIGHT, gguf.iq4_nl_type, 24, 24, 64),
}


def type_fn_of(cfg_kw, dense_fn):
    """(type_fn(name, il), embd_type) of a shape under the 8-expert recipe of a dense one"""
    L, rec = cfg_kw["L"], gguf.mixtral_b32_type(dense_fn)
    fn = lambda name, il: rec(name, il, L)
    return fn, fn("token_embd", 0)


def model_path(cfg, d="/dev/shm"):
    return os.path.join(d, "bamd_fx_moe_b32_%s.gguf" % cfg)


def ensure_model(cfg, d="/dev/shm"):
    kw, ekw, dense_fn = CONFIGS[cfg][:3]
    p = model_path(cfg, d)
    if not os.path.exists(p + ".done"):
        fn, embd = type_fn_of(kw, dense_fn)
        gguf.write_synthetic_llama(p, seed=7, reuse_layers=True, type_fn=fn, embd_type=embd, **ekw, **kw)
        open(p + ".done", "w").write("ok")
    return p


def main():
    import subprocess
    threads = int(os.environ.get("REF_THREADS", str(os.cpu_count() or 8)))
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_run")
    for cfg in sys.argv[1:] or list(CONFIGS):
        n_prompt, n_decode, n_ctx = CONFIGS[cfg][3:]
        p = ensure_model(cfg)
        out = os.path.join(HERE, "moe_b32_%s.bgld" % cfg)
        r = subprocess.run([exe, p, str(threads), str(n_prompt), str(n_decode), str(n_ctx), out], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
        dg, sz = moe.full.file_digest(p)
        line = r.stdout.decode().strip().splitlines()[-1]
        with open(out + ".txt", "w") as f:
            f.write("%s\ngguf_bytes=%d gguf_sha256_first64MiB=%s gguf_xxh3_128=%s\n" % (line, sz, dg, moe.full.file_digest_full(p)))
        print(cfg, line, flush=True)


if __name__ == "__main__":
    main()
