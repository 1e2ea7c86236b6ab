#!/usr/bin/env python3
"""Fixtures of mixture-of-experts models with UNQUANTISED experts (all-F16, all-BF16, all-F32 files: what the converter writes before anything is quantised),
from the GENUINE reference (build container only; needs oracle/_ref/ref_run: `make -C oracle refrun`).  As tests/golden/gen_moe_b32_fixtures.py: the TINY shape,
side-file format and main loop of tests/golden/gen_moe_fixtures.py, with its own CONFIGS.  Committed: DATA ONLY (tests/golden/moe_flt_<cfg>.bgld, a few KB).

    python tests/golden/gen_moe_flt_fixtures.py [cfg ...]
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
    # name: (model kwargs, expert kwargs, the file's one matrix type, n_prompt, n_decode, n_ctx)
    "tiny_f16": (TINY, EIGHT, gguf.F16, 24, 24, 64),
    "tiny_bf16": (TINY, EIGHT, gguf.BF16, 24, 24, 64),
    "tiny_f32": (TINY, EIGHT, gguf.F32, 24, 24, 64),
}


def model_path(cfg, d="/dev/shm"):
    return os.path.join(d, "bamd_fx_moe_flt_%s.gguf" % cfg)


def ensure_model(cfg, d="/dev/shm"):
    kw, ekw, t = CONFIGS[cfg][:3]
    p = model_path(cfg, d)
    if not os.path.exists(p + ".done"):
        rec = gguf.mixtral_float_type(t)
        gguf.write_synthetic_llama(p, seed=7, reuse_layers=True, type_fn=lambda name, il: rec(name, il, kw["L"]), embd_type=t, **ekw, **kw)
        open(p + ".done", "w").write("ok")
    return p


def main():
    import subprocess
    threads = int(os.environ.get("REF_THREADS", str(os.cpu_count() or 8)))
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_run")
    for cfg in sys.argv[1:] or list(CONFIGS):
        n_prompt, n_decode, n_ctx = CONFIGS[cfg][3:]
        p = ensure_model(cfg)
        out = os.path.join(HERE, "moe_flt_%s.bgld" % cfg)
        r = subprocess.run([exe, p, str(threads), str(n_prompt), str(n_decode), str(n_ctx), out], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
        dg, sz = moe.full.file_digest(p)
        line = r.stdout.decode().strip().splitlines()[-1]
        with open(out + ".txt", "w") as f:
            f.write("%s\ngguf_bytes=%d gguf_sha256_first64MiB=%s gguf_xxh3_128=%s\n" % (line, sz, dg, moe.full.file_digest_full(p)))
        print(cfg, line, flush=True)


if __name__ == "__main__":
    main()
