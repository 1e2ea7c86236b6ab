#!/usr/bin/env python3
"""Fixtures of mixture-of-experts models with Q3_K / Q2_K / IQ4_XS experts, from the GENUINE reference (build container only; needs oracle/_ref/ref_run:
`make -C oracle refrun`).  As tests/golden/gen_moe_b32_fixtures.py, whose TINY shape, 8-expert recipes (booster_amd.gguf.mixtral_b32_type), model writer and
side-file format this generator shares, with its own CONFIGS.  Committed: DATA ONLY (tests/golden/moe_kq_<cfg>.bgld, a few KB): python tests/golden/gen_moe_kq_fixtures.py [cfg ...]"""
import importlib.util
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("gen_moe_b32_fixtures", os.path.join(HERE, "gen_moe_b32_fixtures.py"))
b32 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(b32)
gguf, moe = b32.gguf, b32.moe

CONFIGS = {
    # name: (model kwargs, expert kwargs, dense recipe of the ftype, n_prompt, n_decode, n_ctx); L = 8: n_layer / 16 = 0, n_layer / 8 = 1
    # Q3_K | Q8_0 | Q8_0 QKV, Q5_K attn_output, Q3_K gate / up experts beside Q4_K down experts
    "tiny_q3_k_m": (b32.TINY, b32.EIGHT, gguf.q3_k_m_type, 24, 24, 64),
    # Q2_K | Q8_0 | Q8_0 QKV, Q5_K attn_output, Q2_K gate / up experts beside Q3_K down experts
    "tiny_q2_k": (b32.TINY, b32.EIGHT, gguf.q2_k_type, 24, 24, 64),
    # IQ4_XS | Q8_0 | Q8_0 QKV, Q5_K attn_output, IQ4_XS gate / up experts, Q5_K down experts in layer 0 and IQ4_XS ones behind it
    "tiny_iq4_xs": (b32.TINY, b32.EIGHT, gguf.iq4_xs_type, 24, 24, 64),
}
b32.CONFIGS.update(CONFIGS)      # ensure_model writes bamd_fx_moe_b32_<cfg>.gguf from these entries
ensure_model, model_path = b32.ensure_model, b32.model_path


def main():
    threads = int(os.environ.get("REF_THREADS", str(os.cpu_count() or 8)))
    exe = os.path.join(b32.ROOT, "oracle", "_ref", "ref_run")
    for cfg in sys.argv[1:] or list(CONFIGS):
        n_prompt, n_decode, n_ctx = CONFIGS[cfg][3:]
        p = b32.ensure_model(cfg)
        out = os.path.join(HERE, "moe_kq_%s.bgld" % cfg)
        r = subprocess.run([exe, p, str(threads), str(n_prompt), str(n_decode), str(n_ctx), out], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
        dg, sz = moe.full.file_digest(p)
        line = r.stdout.decode().strip().splitlines()[-1]
        with open(out + ".txt", "w") as f:
            f.write("%s\ngguf_bytes=%d gguf_sha256_first64MiB=%s gguf_xxh3_128=%s\n" % (line, sz, dg, moe.full.file_digest_full(p)))
        print(cfg, line, flush=True)


if __name__ == "__main__":
    main()
