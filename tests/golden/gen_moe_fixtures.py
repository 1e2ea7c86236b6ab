#!/usr/bin/env python3
"""Mixture-of-experts model fixtures from the GENUINE reference (build container only; needs oracle/_ref/ref_run: `make -C oracle refrun`).

As tests/golden/gen_iq4xs_fixtures.py — whose digests and .bgld + side-file format this generator shares — with its own CONFIGS: the deterministic synthetic
GGUF of each shape with llama.expert_count experts per layer (booster_amd.gguf.write_synthetic_llama(n_expert=..)), evaluated by the reference CPU path
(llm_build_moe_ffn) on the synthetic prompt tok[i] = (7919 i + 13) mod V, greedy.
Committed: DATA ONLY (tests/golden/moe_<cfg>.bgld, a few KB).

    python tests/golden/gen_moe_fixtures.py [cfg ...]
"""
import importlib.util
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from booster_amd import gguf  # noqa: E402

_spec = importlib.util.spec_from_file_location("gen_fullsize_fixtures", os.path.join(HERE, "gen_fullsize_fixtures.py"))
full = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(full)

TINY = dict(E=512, H=8, Hkv=2, L=8, F=768, V=512, theta=500000.0)
CONFIGS = {
    # name: (model kwargs, expert kwargs, recipe, n_prompt, n_decode, n_ctx)
    # the 8-expert Q4_K_M recipe: Q4_K | Q8_0 | Q8_0 QKV (two launches), Q5_K attn_output, Q6_K and Q4_K down experts in different layers
    "tiny_mixtral": (TINY, dict(n_expert=8, n_expert_used=2), "mixtral", 24, 24, 64),
    # 16 experts, 4 used: the n_expert == 8 rules do not apply — the dense Q4_K_M types, a uniform Q4_K QKV where attn_v is not Q6_K
    "tiny_moe16": (TINY, dict(n_expert=16, n_expert_used=4), "dense", 24, 24, 64),
    # two layers at the 8x7B widths: K = 4096 and the down experts at K = 14336 (56 records), two 16 KB activation blobs in the down launch
    "mixw_moe": (dict(E=4096, H=32, Hkv=8, L=2, F=14336, V=32000, theta=1000000.0), dict(n_expert=8, n_expert_used=2), "mixtral", 32, 16, 128),
}


def type_fn_of(cfg_kw, recipe):
    """(type_fn(name, il), embd_type) of a shape under its recipe"""
    L = cfg_kw["L"]
    if recipe == "mixtral":
        fn = lambda name, il: gguf.mixtral_q4_k_m_type(name, il, L)
    else:
        fn = lambda name, il: gguf.F32 if name == "ffn_gate_inp" else gguf.q4_k_m_type(name.replace("_exps", ""), il, L)
    return fn, fn("token_embd", 0)


def model_path(cfg, d="/dev/shm"):
    return os.path.join(d, "bamd_fx_moe_%s.gguf" % cfg)


def ensure_model(cfg, d="/dev/shm"):
    kw, ekw, recipe = CONFIGS[cfg][0], CONFIGS[cfg][1], CONFIGS[cfg][2]
    p = model_path(cfg, d)
    if not os.path.exists(p + ".done"):
        fn, embd = type_fn_of(kw, recipe)
        gguf.write_synthetic_llama(p, seed=7, reuse_layers=True, type_fn=fn, embd_type=embd, **ekw, **kw)
        open(p + ".done", "w").write("ok")
    return p


def main():
    cfgs = sys.argv[1:] or list(CONFIGS)
    threads = int(os.environ.get("REF_THREADS", str(os.cpu_count() or 8)))
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_run")
    for cfg in cfgs:
        n_prompt, n_decode, n_ctx = CONFIGS[cfg][3:]
        p = ensure_model(cfg)
        out = os.path.join(HERE, "moe_%s.bgld" % cfg)
        t0 = time.time()
        r = subprocess.run([exe, p, str(threads), str(n_prompt), str(n_decode), str(n_ctx), out], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
        dg, sz = full.file_digest(p)
        line = r.stdout.decode().strip().splitlines()[-1]
        with open(out + ".txt", "w") as f:
            f.write("%s\ngguf_bytes=%d gguf_sha256_first64MiB=%s gguf_xxh3_128=%s\n" % (line, sz, dg, full.file_digest_full(p)))
        print(cfg, line, "(%.0f s)" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
