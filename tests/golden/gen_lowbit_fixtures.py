#!/usr/bin/env python3
"""Full-size Q3_K_M / Q2_K fixtures from the GENUINE reference (build container only; needs oracle/_ref/ref_run: `make -C oracle refrun`).

As tests/golden/gen_fullsize_fixtures.py — whose model writer, digests and .bgld + side-file format this generator shares — with its own CONFIGS: the
deterministic synthetic GGUF of each shape under llama.cpp's Q3_K_M / Q2_K recipe (booster_amd.gguf.q3_k_m_type / q2_k_type, token_embd in the base type),
evaluated by the reference CPU path on the synthetic prompt tok[i] = (7919 i + 13) mod V, greedy.  Committed: DATA ONLY (tests/golden/lowbit_<cfg>.bgld, a few KB).

    python tests/golden/gen_lowbit_fixtures.py [cfg ...]      cfg in: 8b_q3_k_m 8b_q2_k l2_7b_q2_k 8bw_q2_k_mix tiny_q3_k_m tiny_q2_k
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

L3_8B = dict(E=4096, H=32, Hkv=8, L=32, F=14336, V=128256, theta=500000.0)
CONFIGS = {
    # name: (model kwargs, recipe, n_prompt, n_decode, n_ctx)
    "8b_q3_k_m": (L3_8B, "q3_k_m", 128, 64, 512),
    # attn_v Q4_K (n_gqa 4), attn_output and ffn_down Q3_K (K = 14336)
    "8b_q2_k": (L3_8B, "q2_k", 128, 64, 512),
    # Llama-2-7B: no GQA, so attn_v is Q3_K; ffn_down Q3_K over 43 super-blocks (uneven split-K shares)
    "l2_7b_q2_k": (dict(E=4096, H=32, Hkv=32, L=32, F=11008, V=32000, theta=10000.0, n_ctx_train=4096), "q2_k", 64, 32, 256),
    # two layers at the 8B widths with the types the recipes do not combine there: attn_v Q3_K beside Q2_K q | k at three row-groups per workgroup (the mixed-type
    # split-K QKV kernel with a Q3_K second segment) and a Q2_K attn_output (the co-launched attention || wo kernel's Q2_K instance)
    "8bw_q2_k_mix": (dict(E=4096, H=32, Hkv=8, L=2, F=14336, V=32000, theta=500000.0), "q2_k_mix", 32, 16, 128),
    # seconds on any machine: the engine path of both recipes (embedding rows, every launch, the batched prompt) at small widths
    "tiny_q3_k_m": (dict(E=512, H=8, Hkv=2, L=3, F=768, V=512, theta=500000.0), "q3_k_m", 24, 24, 64),
    "tiny_q2_k": (dict(E=512, H=8, Hkv=2, L=3, F=768, V=512, theta=500000.0), "q2_k", 24, 24, 64),
}


def type_fn_of(recipe, kw):
    L, n_gqa = kw["L"], kw["H"] // kw["Hkv"]
    if recipe == "q3_k_m":
        return (lambda name, il: gguf.q3_k_m_type(name, il, L)), gguf.Q3_K
    if recipe == "q2_k_mix":
        return (lambda name, il: gguf.Q2_K if name == "attn_output" else gguf.q2_k_type(name, il, L, 1)), gguf.Q2_K
    return (lambda name, il: gguf.q2_k_type(name, il, L, n_gqa)), gguf.Q2_K


def model_path(cfg, d="/dev/shm"):
    return os.path.join(d, "bamd_fx_%s.gguf" % cfg)


def ensure_model(cfg, d="/dev/shm"):
    kw, recipe = CONFIGS[cfg][0], CONFIGS[cfg][1]
    p = model_path(cfg, d)
    if not os.path.exists(p + ".done"):
        fn, embd = type_fn_of(recipe, kw)
        gguf.write_synthetic_llama(p, seed=7, reuse_layers=True, type_fn=fn, embd_type=embd, **kw)
        open(p + ".done", "w").write("ok")
    return p


def main():
    cfgs = sys.argv[1:] or list(CONFIGS)
    threads = int(os.environ.get("REF_THREADS", str(os.cpu_count() or 8)))
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_run")
    for cfg in cfgs:
        _, _, n_prompt, n_decode, n_ctx = CONFIGS[cfg]
        p = ensure_model(cfg)
        out = os.path.join(HERE, "lowbit_%s.bgld" % cfg)
        t0 = time.time()
        r = subprocess.run([exe, p, str(threads), str(n_prompt), str(n_decode), str(n_ctx), out], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
        dg, sz = full.file_digest(p)
        line = r.stdout.decode().strip().splitlines()[-1]
        with open(out + ".txt", "w") as f:
            f.write("%s\ngguf_bytes=%d gguf_sha256_first64MiB=%s gguf_xxh3_128=%s\n" % (line, sz, dg, full.file_digest_full(p)))
        print(cfg, line, "(%.0f s)" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
