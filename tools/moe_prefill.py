"""Prompt rate of the synthetic Mixtral-8x7B-shaped file of tools/moe_decode.py (E 4096, F 14336, L 32, 8 experts, 2 used, the 8-expert Q4_K_M recipe): a
2048-token prompt at n_past = 0, evaluated batched (micro-batches of 512 through the grouped expert mat-muls of bamd_moe_batch.hip) and token by token
(set_prefill_batch(False): the routed decode launches), the two alternating in one process, five each after a warm-up of both — medians and ranges in tok/s.
Then the same alternation for prompts of 2, 4, 8 and 16 tokens: where the batched path stops paying, if it does.  GPU box only.  The times of the seven
launches per layer come from a run of its own under the profiler's kernel trace (--once: one batched 512-token micro-batch, eager, every launch a kernel of a
stable name).

    python tools/moe_prefill.py [--once]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from moe_decode import b, gen  # noqa: E402  (its 8x7b entry of the generator's CONFIGS)


def rate(ctx, prompt, batched):
    """tok/s of evaluating `prompt` at n_past = 0 (decode returns with the logits on the host); short prompts twenty times over, for a window worth timing"""
    b.set_prefill_batch(batched)
    inner = 1 if len(prompt) >= 256 else 20
    t0 = time.perf_counter()
    for _ in range(inner):
        ctx.decode(prompt, 0)
    return inner * len(prompt) / (time.perf_counter() - t0)


def alternate(ctx, prompt, reps=5):
    got = {True: [], False: []}
    for rep in range(reps + 1):                               # (rep 0: the warm-up of both)
        for batched in (True, False):
            r = rate(ctx, prompt, batched)
            if rep:
                got[batched].append(r)
    return got


def main():
    m = b.Model(gen.ensure_model("8x7b"))
    ctx = b.Context(m, 2048)
    prompt = [(7919 * i + 13) % m.n_vocab for i in range(2048)]
    try:
        if "--once" in sys.argv:
            ctx.decode(prompt[:512], 0)
            return
        for n in (2048, 2, 4, 8, 16):
            got = alternate(ctx, prompt[:n])
            for batched, name in ((True, "batched"), (False, "token by token")):
                r = got[batched]
                print("prompt of %4d tokens, %-14s median %8.1f tok/s  (range %.1f - %.1f, 5 alternating evaluations after a warm-up)"
                      % (n, name, statistics.median(r), min(r), max(r)), flush=True)
    finally:
        b.set_prefill_batch(True)
        ctx.close(); m.close()


if __name__ == "__main__":
    main()
