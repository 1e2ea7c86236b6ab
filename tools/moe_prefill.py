"""Prompt rate of the synthetic Mixtral-8x7B-shaped file of tools/moe_decode.py (E 4096, F 14336, L 32, 8 experts, 2 used, the 8-expert Q4_K_M recipe): a
2048-token prompt at n_past = 0, evaluated batched (micro-batches of 512 through the grouped expert mat-muls of bamd_moe_batch.hip) and token by token
(set_prefill_batch(False): the routed decode launches), the two alternating in one process, five each after a warm-up of both — medians and ranges in tok/s.
Then the same alternation for prompts of 2, 4, 8 and 16 tokens: where the batched path stops paying, if it does.  GPU box only.  The times of the seven
launches per layer come from a run of its own under the profiler's kernel trace (--once: one batched 512-token micro-batch, eager, every launch a kernel of a
stable name).

--moe: the matrix-core path of the grouped expert mat-muls (bamd_moe_batch_mfma.hip, bamd_moe_batch_kq_mfma.hip, bamd_moe_batch_b32_mfma.hip) against the integer-dot one.  Side tables are decided at model load, so
the file is loaded twice, with set_prefill_moe(False) and (True) — set_prefill_q0(True) in both arms: the recipe's Q8_0 attn_k / attn_v — and batched prompts of
2048, 8, 16, 32, 64, 128 and 512 tokens alternate between the two models; the side-table bytes and the free memory around the second load are printed.  With
--once: one 512-token micro-batch of the model with tables.

--recipe NAME[,NAME..]: the same measurement under other 8-expert recipes, one after another (tools/moe_decode.py lists them); experts of the 32-weight block
formats take the grouped mat-muls of bamd_moe_batch_b32.hip.  With --moe: the two arms of that recipe's file, its family switches (SWITCHES below) on in BOTH
arms — such experts, and Q3_K / Q2_K / IQ4_XS ones (recipes q3_k_m, q2_k, iq4_xs: switches lowbit / xs), go to the matrix cores only while set_prefill_moe AND
their own family's switch are on.

    python tools/moe_prefill.py [--moe] [--once] [--recipe q4_k_m,q4_0,q8_0]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from moe_decode import b, model_of, recipes  # noqa: E402  (the 8x7b entries of the generators' CONFIGS)


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


# the family switches a recipe's file needs beside set_prefill_moe for its side tables (all or nothing per model): q0 for the Q8_0 attn_k / attn_v of every recipe
SWITCHES = {"q4_k_m": ("q0",), "q4_0": ("q0",), "q5_0": ("q0",), "q8_0": ("q0",), "q4_1": ("q0", "q1"), "q5_1": ("q0", "q1"), "iq4_nl": ("q0", "nl"),
            "q3_k_m": ("q0", "lowbit"), "q2_k": ("q0", "lowbit"), "iq4_xs": ("q0", "xs")}


def main_moe(recipe):
    path, arms = model_of(recipe), {}
    for name in SWITCHES[recipe]:
        getattr(b, "set_prefill_" + name)(True)
    print("recipe %s, switches on in both arms: %s" % (recipe, ", ".join(SWITCHES[recipe])), flush=True)
    try:
        for on in (False, True) if "--once" not in sys.argv else (True,):
            b.set_prefill_moe(on)
            free0 = torch_free()
            m = b.Model(path)
            arms[on] = (m, b.Context(m, 2048))
            print("set_prefill_moe(%s): side tables %.2f GiB, device memory free before the load %.2f GiB, after %.2f GiB"
                  % (on, m.prefill_aux_bytes() / 2.0 ** 30, free0 / 2.0 ** 30, torch_free() / 2.0 ** 30), flush=True)
        prompt = [(7919 * i + 13) % arms[True][0].n_vocab for i in range(2048)]
        if "--once" in sys.argv:
            arms[True][1].decode(prompt[:512], 0)
            return
        for n in (2048, 8, 16, 32, 64, 128, 512):
            got = {False: [], True: []}
            for rep in range(6):                              # (rep 0: the warm-up of both)
                for on in (False, True):
                    b.set_prefill_moe(on)
                    runs = b.moe_batch_mfma_runs()
                    r = rate(arms[on][1], prompt[:n], True)
                    assert (b.moe_batch_mfma_runs() > runs) == on
                    if rep:
                        got[on].append(r)
            for on, name in ((False, "integer-dot"), (True, "matrix cores")):
                print("prompt of %4d tokens, experts on %-12s median %8.1f tok/s  (range %.1f - %.1f, 5 alternating evaluations after a warm-up)"
                      % (n, name, statistics.median(got[on]), min(got[on]), max(got[on])), flush=True)
    finally:
        for name in ("moe",) + SWITCHES[recipe]:
            getattr(b, "set_prefill_" + name)(os.environ.get("BAMD_PREFILL_" + name.upper(), "")[:1] == "1")
        for m, ctx in arms.values():
            ctx.close(); m.close()


def torch_free():
    import torch
    return torch.cuda.mem_get_info()[0]


def main():
    for recipe in recipes():
        main_moe(recipe) if "--moe" in sys.argv else main_recipe(recipe)


def main_recipe(recipe):
    m = b.Model(model_of(recipe))
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
                print("%-7s prompt of %4d tokens, %-14s median %8.1f tok/s  (range %.1f - %.1f, 5 alternating evaluations after a warm-up)"
                      % (recipe, n, name, statistics.median(r), min(r), max(r)), flush=True)
    finally:
        b.set_prefill_batch(True)
        ctx.close(); m.close()


if __name__ == "__main__":
    main()
