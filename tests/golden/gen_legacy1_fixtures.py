#!/usr/bin/env python3
"""Q4_1 / Q5_1 model fixtures from the GENUINE reference (build container only; needs oracle/_ref/ref_run: `make -C oracle refrun`).

As tests/golden/gen_legacy_fixtures.py — whose model writer, digests and .bgld + side-file format this generator shares (tests/golden/gen_lowbit_fixtures.py's) —
with its own CONFIGS: the deterministic synthetic GGUF of each shape under llama.cpp's Q4_1 / Q5_1 recipe (booster_amd.gguf.q4_1_type / q5_1_type: every matrix and
token_embd in the base type, output.weight Q6_K) or under its Q4_0 / Q5_0 recipe with an importance matrix (q4_0_imatrix_type / q5_0_imatrix_type: ffn_down of
the first n_layer / 8 layers Q4_1 / Q5_1), evaluated by the reference CPU path on the synthetic prompt tok[i] = (7919 i + 13) mod V, greedy.
Committed: DATA ONLY (tests/golden/legacy1_<cfg>.bgld, a few KB).

    python tests/golden/gen_legacy1_fixtures.py [cfg ...]
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

TINY = dict(E=512, H=8, Hkv=2, L=3, F=768, V=512, theta=500000.0)
TINY8 = dict(TINY, L=8)                          # n_layer // 8 = 1: layer 0 carries the "_1" ffn_down of the importance-matrix recipes
W8B = dict(E=4096, H=32, Hkv=8, L=2, F=14336, V=32000, theta=500000.0)
CONFIGS = {
    # name: (model kwargs, recipe, n_prompt, n_decode, n_ctx)
    # seconds on any machine: embedding rows, every launch, the batched prompt at small widths
    "tiny_q4_1": (TINY, "q4_1", 24, 24, 64),
    "tiny_q5_1": (TINY, "q5_1", 24, 24, 64),
    # a Q4_0 / Q5_0 model whose first layer's ffn_down is Q4_1 / Q5_1, lm_head Q6_K: three activation forms in one step
    "tiny_q4_0_imat": (TINY8, "q4_0_imatrix", 24, 24, 64),
    "tiny_q5_0_imat": (TINY8, "q5_0_imatrix", 24, 24, 64),
    # two layers at the 8B widths: K = 4096 (16 records, the co-launched wo) and ffn_down at K = 14336 (56 records); Q6_K lm_head with its arg-max epilogue
    "8bw_q4_1": (W8B, "q4_1", 32, 16, 128),
    "8bw_q5_1": (W8B, "q5_1", 32, 16, 128),
}
L3_8B = dict(E=4096, H=32, Hkv=8, L=32, F=14336, V=128256, theta=500000.0)
RECIPES = {"q4_1": gguf.q4_1_type, "q5_1": gguf.q5_1_type, "q4_0_imatrix": gguf.q4_0_imatrix_type, "q5_0_imatrix": gguf.q5_0_imatrix_type}


def type_fn_of(recipe, kw):
    L, rf = kw["L"], RECIPES[recipe]
    return (lambda name, il: rf(name, il, L)), rf("token_embd", 0, L)


def model_path(cfg, d="/dev/shm"):
    return os.path.join(d, "bamd_fx_legacy1_%s.gguf" % cfg)


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
        out = os.path.join(HERE, "legacy1_%s.bgld" % cfg)
        t0 = time.time()
        r = subprocess.run([exe, p, str(threads), str(n_prompt), str(n_decode), str(n_ctx), out], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
        dg, sz = full.file_digest(p)
        line = r.stdout.decode().strip().splitlines()[-1]
        with open(out + ".txt", "w") as f:
            f.write("%s\ngguf_bytes=%d gguf_sha256_first64MiB=%s gguf_xxh3_128=%s\n" % (line, sz, dg, full.file_digest_full(p)))
        print(cfg, line, "(%.0f s)" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
