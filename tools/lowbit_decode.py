"""Greedy decode rate of the synthetic Llama-3-8B file under the Q3_K_M and Q2_K recipes beside the Q4_K_M file, and with --prompt N the prompt rate of the
three files: with the switch at its default (Q3_K_M / Q2_K on the integer-dot kernel) and, where the library has it, with set_prefill_lowbit(True) (their
matrix-core kernels).  GPU box only.  Decode: per file a 128-token prompt, then generate_greedy of 128 steps, five repetitions; prompt: three repetitions after
a warm-up — median and range.

    python tools/lowbit_decode.py [--prompt 2048] [--only-prompt]
"""
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import booster_amd as b  # noqa: E402
from booster_amd import gguf  # noqa: E402

_spec = importlib.util.spec_from_file_location("gen_lowbit_fixtures", os.path.join(ROOT, "tests", "golden", "gen_lowbit_fixtures.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


def q4_k_m_file():
    p = gen.full.model_path("8b")
    if not os.path.exists(p + ".done"):
        gguf.write_synthetic_llama(p, seed=7, reuse_layers=True, **gen.L3_8B)
        open(p + ".done", "w").write("ok")
    return p


def decode_rate(path, n_prompt=128, n_steps=128, reps=5, n_ctx=512):
    m = b.Model(path)
    ctx = b.Context(m, n_ctx)
    prompt = [(7919 * i + 13) % m.n_vocab for i in range(n_prompt)]
    rates = []
    for _ in range(reps + 1):                                   # the first repetition warms up (graph capture, clocks)
        b.lib().bamd_kv_cache_clear(ctx.h)
        ctx.decode(prompt, 0)
        _, ms = ctx.generate_greedy(n_prompt, n_steps)
        rates.append(n_steps / ms * 1e3)
    ctx.close(); m.close()
    return rates[1:]


def prompt_rate(path, n_prompt, reps=3):
    m = b.Model(path)
    ctx = b.Context(m, 4096)
    prompt = [(7919 * i + 13) % m.n_vocab for i in range(n_prompt)]
    aux = m.prefill_aux_bytes() if hasattr(m, "prefill_aux_bytes") else -1
    rates = []
    for _ in range(reps + 1):
        b.lib().bamd_kv_cache_clear(ctx.h)
        t0 = time.perf_counter()
        for i in range(0, n_prompt, 512):
            ctx.decode(prompt[i:i + 512], i)
        rates.append(n_prompt / (time.perf_counter() - t0))
    ctx.close(); m.close()
    return rates[1:], aux


def main():
    files = [("Q4_K_M", q4_k_m_file()), ("Q3_K_M", gen.ensure_model("8b_q3_k_m")), ("Q2_K", gen.ensure_model("8b_q2_k"))]
    for name, p in [] if "--only-prompt" in sys.argv else files:
        r = decode_rate(p)
        print("decode %-7s %5.2f GB: median %7.1f tok/s  (range %.1f - %.1f, 5 x 128 steps after a 128-token prompt)" % (name, os.path.getsize(p) / 1e9, statistics.median(r), min(r), max(r)), flush=True)
    # Llama-2-7B widths: no GQA (attn_v Q3_K under Q2_K), n_ff 11008 = 43 super-blocks; its gate/up launch (1376 row-groups) has no seven-pair shape
    for name, p in () if "--only-prompt" in sys.argv else (("Q4_K_M", gen.full.ensure_model("l2_7b")), ("Q2_K", gen.ensure_model("l2_7b_q2_k"))):
        r = decode_rate(p, n_prompt=64, n_ctx=256)
        print("decode Llama-2-7B %-7s %5.2f GB: median %7.1f tok/s  (range %.1f - %.1f, 5 x 128 steps after a 64-token prompt)" % (name, os.path.getsize(p) / 1e9, statistics.median(r), min(r), max(r)), flush=True)
    if "--prompt" in sys.argv:
        n = int(sys.argv[sys.argv.index("--prompt") + 1])
        legs = [(name, p, False) for name, p in files]
        if hasattr(b, "set_prefill_lowbit"):
            legs += [(name, p, True) for name, p in files[1:]]
        for name, p, on in legs:
            if on:
                b.set_prefill_lowbit(True)
            try:
                r, aux = prompt_rate(p, n)
            finally:
                if on:
                    b.set_prefill_lowbit(False)
            how = "matrix-core kernels" if aux > 0 else "integer-dot kernel: the model holds Q3_K / Q2_K matrices" if aux == 0 else "a library without prefill_aux_bytes: side tables unknown"
            print("prompt %-7s %d tokens, low-bit switch %s: median %7.1f tok/s  (range %.1f - %.1f; %s, side tables %.2f GiB)" % (name, n, "on" if on else "off", statistics.median(r),
                  min(r), max(r), how, max(aux, 0) / 2 ** 30), flush=True)


if __name__ == "__main__":
    main()
