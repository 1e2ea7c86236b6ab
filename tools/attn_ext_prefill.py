"""Prompt rate with the matrix-core attention of head_dim 64 and gq 3 (bamd_attention_mfma_ext.hip, set_attn_mfma_ext) against the VALU kernels these shapes run on
by default: synthetic files of the Llama-3.2-1B shape (E 2048, H 32, Hkv 8: head_dim 64, gq 4; L 16, F 8192) and the Llama-3.2-3B shape (E 3072, H 24, Hkv 8:
head_dim 128, gq 3; L 28, F 8192) under the Q4_K_M recipe (write_synthetic_llama, reuse_layers=True, a vocabulary of 32 768).  A 2048-token prompt at n_past = 0 in
a context of 4096, then prompts of 64, 128, 256 and 512 tokens (the short ones twenty evaluations per timing: from what length the matrix-core kernel wins), the switch alternating off / on in one process and one context — it is read at each launch —:
five evaluations each after a warm-up of both, medians and ranges in tok/s, attn_batch_mfma_runs() per arm, and the logits of the two arms compared as bits.
GPU box only.

    python tools/attn_ext_prefill.py > profiles/attn_mfma_ext.txt
"""
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import booster_amd as b  # noqa: E402
from booster_amd import gguf  # noqa: E402

V = 32768
SHAPES = (("Llama-3.2-1B shape (head_dim 64, gq 4)", dict(E=2048, H=32, Hkv=8, L=16, F=8192)),
          ("Llama-3.2-3B shape (head_dim 128, gq 3)", dict(E=3072, H=24, Hkv=8, L=28, F=8192)))


def evaluate(ctx, prompt):
    """(tok/s, logits) of evaluating `prompt` at n_past = 0; a short prompt twenty times over, for a window worth timing"""
    inner = 1 if len(prompt) >= 256 else 20
    t0 = time.perf_counter()
    for _ in range(inner):
        lg = ctx.decode(prompt, 0)
    return inner * len(prompt) / (time.perf_counter() - t0), lg.copy()


def main():
    for name, kw in SHAPES:
        path = os.path.join(tempfile.gettempdir(), "bamd_attn_ext_E%d_H%d.gguf" % (kw["E"], kw["H"]))
        if not os.path.exists(path):
            gguf.write_synthetic_llama(path, V=V, seed=7, reuse_layers=True, **kw)
        m = b.Model(path)
        ctx = b.Context(m, 4096)
        try:
            for n in (2048, 64, 128, 256, 512):
                prompt = [(7919 * i + 13) % V for i in range(n)]
                rates, logits, runs = {False: [], True: []}, {}, {}
                for rep in range(6):                          # (rep 0: the warm-up of both)
                    for on in (False, True):
                        b.set_attn_mfma_ext(on)
                        before = b.attn_batch_mfma_runs()
                        r, logits[on] = evaluate(ctx, prompt)
                        runs[on] = b.attn_batch_mfma_runs() - before
                        if rep:
                            rates[on].append(r)
                same = np.array_equal(logits[False].view(np.uint32), logits[True].view(np.uint32))
                for on in (False, True):
                    print("%s, prompt of %4d tokens, switch %-3s: median %9.1f tok/s  (range %.1f - %.1f, 5 alternating evaluations after a warm-up); "
                          "matrix-core attention launches per timing: %d" % (name, n, "on" if on else "off", statistics.median(rates[on]), min(rates[on]), max(rates[on]), runs[on]), flush=True)
                print("%s, prompt of %4d tokens: on / off = %.3f of the medians; ranges %s; logits of the two arms bit-identical: %s"
                      % (name, n, statistics.median(rates[True]) / statistics.median(rates[False]),
                         "do not overlap" if min(rates[True]) > max(rates[False]) or min(rates[False]) > max(rates[True]) else "OVERLAP", same), flush=True)
                assert same, "the two arms' logits differ"
        finally:
            b.set_attn_mfma_ext(os.environ.get("BAMD_ATTN_MFMA_EXT", "")[:1] == "1")
            ctx.close(); m.close()


if __name__ == "__main__":
    main()
