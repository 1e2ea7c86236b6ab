#!/usr/bin/env python3
"""IQ4_XS model fixtures from the GENUINE reference (build container only; needs oracle/_ref/ref_run: `make -C oracle refrun`).

As tests/golden/gen_iq4nl_fixtures.py — whose model writer, digests and .bgld + side-file format this generator shares — with its own CONFIGS: the deterministic
synthetic GGUF of each shape under llama.cpp's IQ4_XS recipe (booster_amd.gguf.iq4_xs_type: attn_v Q5_K where n_gqa >= 4, ffn_down Q5_K in the layers
il < n_layer / 8 of a file made without an importance matrix, output.weight Q6_K, everything else — token_embd included, unless it is tied — IQ4_XS;
general.file_type 30), evaluated by the reference CPU path on the synthetic prompt tok[i] = (7919 i + 13) mod V, greedy.
Committed: DATA ONLY (tests/golden/<cfg>.bgld, a few KB).

    python tests/golden/gen_iq4xs_fixtures.py [cfg ...]
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
    # name: (model kwargs, recipe kwargs, tied, n_prompt, n_decode, n_ctx)
    # n_gqa 4: Q5_K attn_v beside IQ4_XS attn_q / attn_k, one Q8_K launch with mixed segments; L = 8: layer 0's ffn_down is Q5_K
    "tiny_iq4xs": (TINY, dict(imatrix=False), False, 24, 24, 64),
    # no GQA: a uniform IQ4_XS QKV; an IQ4_XS token_embd
    "tiny_iq4xs_mha": (dict(TINY, Hkv=8), dict(imatrix=False), False, 24, 24, 64),
    # made with an importance matrix: no Q5_K ffn_down; a tied embedding, written Q6_K as the output matrix it also is
    "tiny_iq4xs_imatrix_tied": (TINY, dict(imatrix=True), True, 24, 24, 64),
    # two layers at the 8B widths: K = 4096 (16 records, the co-launched wo) and ffn_down at K = 14336 (56 records); the Q6_K lm_head over V = 32000
    "8bw_iq4xs": (dict(E=4096, H=32, Hkv=8, L=2, F=14336, V=32000, theta=500000.0), dict(imatrix=False), False, 32, 16, 128),
}


def type_fn_of(cfg_kw, recipe_kw, tied=False):
    """(type_fn(name, il), embd_type) of a shape under the IQ4_XS recipe"""
    L, n_gqa = cfg_kw["L"], cfg_kw["H"] // cfg_kw["Hkv"]
    fn = lambda name, il: gguf.iq4_xs_type(name, il, L, n_gqa=n_gqa, **recipe_kw)
    return fn, (fn("output", 0) if tied else fn("token_embd", 0))


def model_path(cfg, d="/dev/shm"):
    return os.path.join(d, "bamd_fx_iq4xs_%s.gguf" % cfg)


def ensure_model(cfg, d="/dev/shm"):
    kw, rkw, tied = CONFIGS[cfg][0], CONFIGS[cfg][1], CONFIGS[cfg][2]
    p = model_path(cfg, d)
    if not os.path.exists(p + ".done"):
        fn, embd = type_fn_of(kw, rkw, tied)
        gguf.write_synthetic_llama(p, seed=7, reuse_layers=True, type_fn=fn, embd_type=embd, tied=tied, file_type=gguf.FTYPE_MOSTLY_IQ4_XS, **kw)
        open(p + ".done", "w").write("ok")
    return p


def main():
    cfgs = sys.argv[1:] or list(CONFIGS)
    threads = int(os.environ.get("REF_THREADS", str(os.cpu_count() or 8)))
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_run")
    for cfg in cfgs:
        n_prompt, n_decode, n_ctx = CONFIGS[cfg][3:]
        p = ensure_model(cfg)
        out = os.path.join(HERE, "%s.bgld" % cfg)
        t0 = time.time()
        r = subprocess.run([exe, p, str(threads), str(n_prompt), str(n_decode), str(n_ctx), out], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
        dg, sz = full.file_digest(p)
        line = r.stdout.decode().strip().splitlines()[-1]
        with open(out + ".txt", "w") as f:
            f.write("%s\ngguf_bytes=%d gguf_sha256_first64MiB=%s gguf_xxh3_128=%s\n" % (line, sz, dg, full.file_digest_full(p)))
        print(cfg, line, "(%.0f s)" % (time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
