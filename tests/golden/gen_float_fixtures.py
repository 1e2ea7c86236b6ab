#!/usr/bin/env python3
"""F16 / BF16 / F32 model fixtures from the GENUINE reference (build container only; needs oracle/_ref/ref_run: `make -C oracle refrun`).

As tests/golden/gen_legacy_fixtures.py — whose model writer, digests and .bgld + side-file format this generator shares — with its own CONFIGS: the deterministic
synthetic GGUF of each shape as convert_hf_to_gguf writes it before anyone quantises (booster_amd.gguf.f16_type / bf16_type / f32_type: every matrix, token_embd
and output.weight in the type, norms f32), and the Q4_K_M recipe with a tied F16 token_embd (an F16 lm_head beside Q8_K-activation layers), evaluated by the
reference CPU path on the synthetic prompt tok[i] = (7919 i + 13) mod V, greedy.  Committed: DATA ONLY (tests/golden/float_<cfg>.bgld, a few KB).

    python tests/golden/gen_float_fixtures.py [cfg ...]
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
W8B = dict(E=4096, H=32, Hkv=8, L=2, F=14336, V=32000, theta=500000.0)
W8B_F32 = dict(E=4096, H=32, Hkv=8, L=1, F=14336, V=8192, theta=500000.0)
CONFIGS = {
    # name: (model kwargs, recipe, n_prompt, n_decode, n_ctx)
    "tiny_f16": (TINY, "f16", 24, 24, 64),
    "tiny_bf16": (TINY, "bf16", 24, 24, 64),
    "tiny_f32": (TINY, "f32", 24, 24, 64),
    # two layers at the 8B widths: K = 4096 and ffn_down at K = 14336; the float lm_head with its arg-max epilogue over 32000 rows
    "8bw_f16": (W8B, "f16", 32, 16, 128),
    "8bw_bf16": (W8B, "bf16", 32, 16, 128),
    # one layer at those widths in F32 (4 bytes per weight: 8 KiB records, half a record per chunk)
    "8bw_f32": (W8B_F32, "f32", 32, 16, 128),
    # the Q4_K_M recipe with an F16 token_embd and no output.weight: the tied F16 lm_head (f32 activations) beside Q8_K-activation layers
    "tiny_q4k_f16embd": (dict(TINY, tied=True), "q4k_f16embd", 24, 24, 64),
}
RECIPES = {"f16": gguf.f16_type, "bf16": gguf.bf16_type, "f32": gguf.f32_type, "q4k_f16embd": gguf.q4_k_m_type}
EMBD = {"f16": gguf.F16, "bf16": gguf.BF16, "f32": gguf.F32, "q4k_f16embd": gguf.F16}


def type_fn_of(recipe, kw):
    L, rf = kw["L"], RECIPES[recipe]
    return (lambda name, il: rf(name, il, L)), EMBD[recipe]


def model_path(cfg, d="/dev/shm"):
    return os.path.join(d, "bamd_fx_float_%s.gguf" % cfg)


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
        out = os.path.join(HERE, "float_%s.bgld" % cfg)
        t0 = time.time()
        r = subprocess.run([exe, p, str(threads), str(n_prompt), str(n_decode), str(n_ctx), out], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
        dg, sz = full.file_digest(p)
        line = r.stdout.decode().strip().splitlines()[-1]
        with open(out + ".txt", "w") as f:
            f.write("%s\ngguf_bytes=%d gguf_sha256_first64MiB=%s gguf_xxh3_128=%s\n" % (line, sz, dg, full.file_digest_full(p)))
        print(cfg, line, "(%.0f s)" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
