"""Greedy decode rate and prompt rate of the synthetic Llama-3-8B file under the Q8_0, Q4_0 and Q5_0 recipes beside the Q4_K_M file, in one job on one card.
GPU box only.  Decode: per file a 128-token prompt, then generate_greedy of 128 steps, five repetitions after a warm-up.  Prompt: N tokens in micro-batches of
512; per Q8_0 / Q4_0 / Q5_0 file one model loaded with the switch off (integer-dot kernel) and one with set_prefill_q0(True) (side tables, matrix-core kernel),
five repetitions each after a warm-up, ALTERNATING between the two; the Q4_K_M file beside them — median and range, and whether the switched-on median clears
the switched-off maximum by more than the switched-off spread.

    python tools/legacy_decode.py [--prompt 2048] [--only-prompt]

--legacy1: the Q4_1 and Q5_1 recipes instead (full depth, synthetic files of tests/golden/gen_legacy1_fixtures.py's writer) beside Q4_0 and Q4_K_M.  Their prompt
lines alternate set_prefill_q1(False) / (True) like the lines above, and two more lines take the Q4_0 file made with an importance matrix (ffn_down of its first
four layers is Q4_1): once with both switches on against both off, once with only set_prefill_q0(True) — no side tables, so it must read like switched off.

    python tools/legacy_decode.py --legacy1 [--prompt 2048] [--only-prompt]

--iq4nl: the IQ4_NL recipe (full depth, synthetic files of tests/golden/gen_iq4nl_fixtures.py's writer) beside Q4_0 and Q4_K_M: the 8B shape as the recipe
writes it (n_gqa 4: Q5_K attn_v, so the QKV of a layer is two launches, six launches per layer) and a uniform-QKV variant of the same shape (attn_v IQ4_NL like
attn_q / attn_k: one QKV launch) — the difference between the two is what the second QKV launch costs per token.  The prompt lines of the two IQ4_NL files
alternate set_prefill_nl(False) / (True) like the lines above (integer-dot kernel against the matrix-core kernel, bamd_prefill2_b32.hip), beside the Q4_0
file under set_prefill_q0 as the nearest twin and the Q4_K_M file.

    python tools/legacy_decode.py --iq4nl [--prompt 2048] [--only-prompt]
    python tools/legacy_decode.py --iq4xs [--prompt 2048] [--only-prompt]
"""
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import booster_amd as b  # noqa: E402
from booster_amd import gguf  # noqa: E402
from lowbit_decode import decode_rate, prompt_rate, q4_k_m_file  # noqa: E402

_spec = importlib.util.spec_from_file_location("gen_legacy_fixtures", os.path.join(ROOT, "tests", "golden", "gen_legacy_fixtures.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
gen.CONFIGS.setdefault("8b_q5_0", (gen.L3_8B, "q5_0", 128, 64, 512))          # a model only: no fixture of it is stored


def set_switches(q0, q1, nl=False):
    b.set_prefill_q0(bool(q0)); b.set_prefill_q1(bool(q1)); b.set_prefill_nl(bool(nl))


def prompt_pair(path, n_prompt, reps=5, q0=True, q1=False, tables=True, nl=False):
    """switched-off and switched-on rates of one file, alternating: ([off], [on], side-table bytes of the switched-on model).  q0 / q1 / nl: what "on" sets;
    tables: whether "on" is enough for this file to get side tables"""
    set_switches(False, False); m0 = b.Model(path)
    set_switches(q0, q1, nl)
    try:
        m1 = b.Model(path)
    finally:
        set_switches(False, False)                              # a model keeps the tables it built at load
    assert m0.prefill_aux_bytes() == 0 and (m1.prefill_aux_bytes() > 0) == tables
    ctxs = [b.Context(m0, 4096), b.Context(m1, 4096)]
    prompt = [(7919 * i + 13) % m0.n_vocab for i in range(n_prompt)]
    rates = ([], [])
    for rep in range(reps + 1):                                 # the first pair warms up
        for k, ctx in enumerate(ctxs):
            set_switches(q0 and k, q1 and k, nl and k)                 # the routing asks the switches as well as the tables
            b.lib().bamd_kv_cache_clear(ctx.h)
            t0 = time.perf_counter()
            for i in range(0, n_prompt, 512):
                ctx.decode(prompt[i:i + 512], i)
            if rep:
                rates[k].append(n_prompt / (time.perf_counter() - t0))
    set_switches(False, False)
    aux = m1.prefill_aux_bytes()
    for c in ctxs:
        c.close()
    m0.close(); m1.close()
    return rates[0], rates[1], aux


def print_pair(name, n, off, on, aux):
    bar = max(off) + (max(off) - min(off))
    print("prompt %-18s %d tokens: switch off median %7.1f tok/s (range %.1f - %.1f; integer-dot kernel) | switch on median %7.1f tok/s (range %.1f - %.1f; %s, "
          "side tables %.2f GiB) | x %.2f | bar (off max + off spread) %.1f: %s" % (name, n, statistics.median(off), min(off), max(off), statistics.median(on), min(on), max(on),
          "matrix-core kernel" if aux > 0 else "integer-dot kernel", aux / 2 ** 30, statistics.median(on) / statistics.median(off), bar, "cleared" if statistics.median(on) > bar else "NOT cleared"), flush=True)


def main_legacy1():
    _s = importlib.util.spec_from_file_location("gen_legacy1_fixtures", os.path.join(ROOT, "tests", "golden", "gen_legacy1_fixtures.py"))
    g1 = importlib.util.module_from_spec(_s)
    _s.loader.exec_module(g1)
    g1.CONFIGS["8b_q4_1"] = (g1.L3_8B, "q4_1", 128, 64, 512)                   # models only: no fixture of them is stored
    g1.CONFIGS["8b_q5_1"] = (g1.L3_8B, "q5_1", 128, 64, 512)
    g1.CONFIGS["8b_q4_0_imat"] = (g1.L3_8B, "q4_0_imatrix", 128, 64, 512)
    only_prompt = "--only-prompt" in sys.argv
    files = [("Q4_K_M", q4_k_m_file())] + ([] if only_prompt else [("Q4_0", gen.ensure_model("8b_q4_0"))]) + [("Q4_1", g1.ensure_model("8b_q4_1")), ("Q5_1", g1.ensure_model("8b_q5_1"))]
    for name, p in [] if only_prompt else files:
        r = decode_rate(p)
        print("decode %-7s %5.2f GB: median %7.1f tok/s  (range %.1f - %.1f, 5 x 128 steps after a 128-token prompt)" % (name, os.path.getsize(p) / 1e9, statistics.median(r), min(r), max(r)), flush=True)
    if "--prompt" in sys.argv:
        n = int(sys.argv[sys.argv.index("--prompt") + 1])
        for name, p in [f for f in files if f[0] in ("Q4_K_M", "Q4_0")]:
            r, aux = prompt_rate(p, n, reps=5)
            print("prompt %-7s %d tokens: median %7.1f tok/s  (range %.1f - %.1f; %s)" % (name, n, statistics.median(r), min(r), max(r),
                  "matrix-core kernels" if aux > 0 else "integer-dot kernel"), flush=True)
        for name, p in [f for f in files if f[0] in ("Q4_1", "Q5_1")]:
            print_pair(name, n, *prompt_pair(p, n, q0=False, q1=True))
        p = g1.ensure_model("8b_q4_0_imat")
        print_pair("Q4_0 imatrix, both switches", n, *prompt_pair(p, n, q0=True, q1=True))
        print_pair("Q4_0 imatrix, BAMD_PREFILL_Q0 only", n, *prompt_pair(p, n, q0=True, q1=False, tables=False))


def main_iq4nl():
    _s = importlib.util.spec_from_file_location("gen_iq4nl_fixtures", os.path.join(ROOT, "tests", "golden", "gen_iq4nl_fixtures.py"))
    gn = importlib.util.module_from_spec(_s)
    _s.loader.exec_module(gn)
    gn.CONFIGS["8b_iq4nl"] = (gen.L3_8B, dict(imatrix=False), False, 128, 64, 512)                  # models only: no fixture of them is stored
    uniform = os.path.join("/dev/shm", "bamd_fx_iq4nl_8b_iq4nl_uniform.gguf")                      # the recipe at n_gqa 1 on the same shape: attn_v IQ4_NL
    if not os.path.exists(uniform + ".done"):
        L = gen.L3_8B["L"]
        fn = lambda name, il: gguf.iq4_nl_type(name, il, L, n_gqa=1)
        gguf.write_synthetic_llama(uniform, seed=7, reuse_layers=True, type_fn=fn, embd_type=gguf.IQ4_NL, file_type=gguf.FTYPE_MOSTLY_IQ4_NL, **gen.L3_8B)
        open(uniform + ".done", "w").write("ok")
    files = [("Q4_K_M", q4_k_m_file()), ("Q4_0", gen.ensure_model("8b_q4_0")), ("IQ4_NL", gn.ensure_model("8b_iq4nl")), ("IQ4_NL uniform QKV", uniform)]
    med = {}
    for name, p in [] if "--only-prompt" in sys.argv else files:
        r = decode_rate(p)
        med[name] = statistics.median(r)
        print("decode %-18s %5.2f GB: median %7.1f tok/s  (range %.1f - %.1f, 5 x 128 steps after a 128-token prompt)" % (name, os.path.getsize(p) / 1e9, med[name], min(r), max(r)), flush=True)
    if med:
        two, one = 1e6 / med["IQ4_NL"], 1e6 / med["IQ4_NL uniform QKV"]
        print("second QKV launch: %.1f us per token at six launches per layer against %.1f us at five = %.2f us per layer (32 layers; the Q5_K attn_v is also %.1f %% more bytes than an IQ4_NL one)"
              % (two, one, (two - one) / 32, 100.0 * (176 / 256 - 18 / 32) / (18 / 32)), flush=True)
    if "--prompt" in sys.argv:
        n = int(sys.argv[sys.argv.index("--prompt") + 1])
        r, aux = prompt_rate(files[0][1], n, reps=5)
        print("prompt %-18s %d tokens: median %7.1f tok/s  (range %.1f - %.1f; %s)" % (files[0][0], n, statistics.median(r), min(r), max(r),
              "matrix-core kernels" if aux > 0 else "integer-dot kernel"), flush=True)
        print_pair("Q4_0", n, *prompt_pair(files[1][1], n))                    # the nearest twin: the same record, one accumulator set, BAMD_PREFILL_Q0
        for name, p in files[2:]:
            print_pair(name, n, *prompt_pair(p, n, q0=False, nl=True))


def main_iq4xs():
    """--iq4xs: the 8B shape under the IQ4_XS recipe as llama.cpp writes it (Q5_K attn_v, Q5_K ffn_down in layers 0-3, Q6_K output; everything is Q8_K, five
    launches per layer) beside IQ4_NL, Q4_0 and Q4_K_M in the same job; with --prompt N the prompt rate on the integer-dot kernel (the type has no matrix-core
    kernel, so its model builds no side tables) beside Q4_K_M on the matrix cores"""
    def load(name):
        _s = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
        g = importlib.util.module_from_spec(_s)
        _s.loader.exec_module(g)
        return g
    gn, gx = load("gen_iq4nl_fixtures"), load("gen_iq4xs_fixtures")
    gn.CONFIGS["8b_iq4nl"] = (gen.L3_8B, dict(imatrix=False), False, 128, 64, 512)                  # models only: no fixture of them is stored
    gx.CONFIGS["8b_iq4xs"] = (gen.L3_8B, dict(imatrix=False), False, 128, 64, 512)
    only_prompt = "--only-prompt" in sys.argv
    files = [("Q4_K_M", q4_k_m_file())] + ([] if only_prompt else [("Q4_0", gen.ensure_model("8b_q4_0")), ("IQ4_NL", gn.ensure_model("8b_iq4nl"))]) + [("IQ4_XS", gx.ensure_model("8b_iq4xs"))]
    for name, p in [] if only_prompt else files:
        r = decode_rate(p)
        print("decode %-7s %5.2f GB: median %7.1f tok/s  (range %.1f - %.1f, 5 x 128 steps after a 128-token prompt)" % (name, os.path.getsize(p) / 1e9, statistics.median(r), min(r), max(r)), flush=True)
    if "--prompt" in sys.argv:
        n = int(sys.argv[sys.argv.index("--prompt") + 1])
        for name, p in [f for f in files if f[0] in ("Q4_K_M", "IQ4_XS")]:
            r, aux = prompt_rate(p, n, reps=5)
            print("prompt %-7s %d tokens: median %7.1f tok/s  (range %.1f - %.1f; %s)" % (name, n, statistics.median(r), min(r), max(r),
                  "matrix-core kernels" if aux > 0 else "integer-dot kernel"), flush=True)


def main():
    if "--legacy1" in sys.argv:
        return main_legacy1()
    if "--iq4xs" in sys.argv:
        return main_iq4xs()
    if "--iq4nl" in sys.argv:
        return main_iq4nl()
    files = [("Q4_K_M", q4_k_m_file()), ("Q8_0", gen.ensure_model("8b_q8_0")), ("Q4_0", gen.ensure_model("8b_q4_0")), ("Q5_0", gen.ensure_model("8b_q5_0"))]
    for name, p in [] if "--only-prompt" in sys.argv else files:
        r = decode_rate(p)
        print("decode %-7s %5.2f GB: median %7.1f tok/s  (range %.1f - %.1f, 5 x 128 steps after a 128-token prompt)" % (name, os.path.getsize(p) / 1e9, statistics.median(r), min(r), max(r)), flush=True)
    if "--prompt" in sys.argv:
        n = int(sys.argv[sys.argv.index("--prompt") + 1])
        r, _ = prompt_rate(files[0][1], n, reps=5)
        print("prompt %-7s %d tokens: median %7.1f tok/s  (range %.1f - %.1f; matrix-core kernels)" % (files[0][0], n, statistics.median(r), min(r), max(r)), flush=True)
        for name, p in files[1:]:
            print_pair(name, n, *prompt_pair(p, n))


if __name__ == "__main__":
    main()
