"""Greedy decode rate and prompt rate of the synthetic Llama-3-8B file as an unquantised GGUF — F16, BF16 and F32 — beside the Q8_0 file, in one job on one card.
GPU box only.  Decode: per file a 128-token prompt, then generate_greedy of 128 steps, five repetitions after a warm-up.  Prompt: N tokens in micro-batches of
512, five repetitions after a warm-up (Q8_0 on the integer-dot kernel).  An F16 / F32 file is measured with set_prefill_flt, a BF16 file with
set_prefill_bf16, off (VALU kernel) and on (f32 matrix-core kernel, bamd_prefill2_flt.hip / bamd_prefill2_bf16.hip) on ONE model and context — the switch is read
at each launch; for BF16 the workgroups that fell back to the two-rounding step are printed too (prefill_bf16_fallback_tiles; expected 0) —
ALTERNATING between the two, as tools/legacy_decode.py does for its switch: median and range of each, whether the switched-on median clears the switched-off
maximum by more than the switched-off spread, and the share of the f32 MFMA peak (157.3 TFLOP/s) that the layer mat-muls' FLOP over the whole prompt time amount to.
Beside every decode median: the bytes streamed per token (every matrix once) and the share of the 8 TB/s token roofline the rate amounts to.

The F16 and BF16 files have the full shape (V 128256).  The F32 file has V 32000: an F32 lm_head of 128256 x 4096 is 2.1 GB, beyond the 2 GiB cap of a stream
copy, and is refused at load.  Each float file is 16 - 30 GB: it is written, measured and removed again before the next one (--keep: left in place).

    python tools/float_decode.py [--prompt 2048] [--only-prompt] [--types f16,bf16,f32] [--keep]

--only-prompt: no decode rates and no Q8_0 file (profiles/float_prefill.txt is the output of --prompt 2048 --only-prompt).
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
from lowbit_decode import decode_rate, prompt_rate  # noqa: E402

_spec = importlib.util.spec_from_file_location("gen_legacy_fixtures", os.path.join(ROOT, "tests", "golden", "gen_legacy_fixtures.py"))
legacy = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(legacy)

L3_8B = dict(E=4096, H=32, Hkv=8, L=32, F=14336, V=128256, theta=500000.0)
SHAPES = {"f16": (L3_8B, gguf.f16_type, gguf.F16), "bf16": (L3_8B, gguf.bf16_type, gguf.BF16), "f32": (dict(L3_8B, V=32000), gguf.f32_type, gguf.F32)}
HBM_BYTES_PER_S = 8.0e12
MFMA_F32_FLOPS = 157.3e12


def float_file(name, d="/dev/shm"):
    kw, rf, embd = SHAPES[name]
    p = os.path.join(d, "bamd_float_8b_%s.gguf" % name)
    if not os.path.exists(p + ".done"):
        gguf.write_synthetic_llama(p, seed=7, reuse_layers=True, type_fn=lambda n, il: rf(n, il, kw["L"]), embd_type=embd, **kw)
        open(p + ".done", "w").write("ok")
    return p


def prompt_pair(path, n_prompt, reps=5, setter=None, types=(0, 1)):
    """switched-off and switched-on prompt rates of one float file (setter: its family's switch; types: what it counts), alternating on one model and context:
    ([off], [on], matrix-core launches counted while on)"""
    setter = setter or b.set_prefill_flt
    counted = lambda: sum(b.prefill_mfma_runs(t) for t in types)
    m = b.Model(path)
    ctx = b.Context(m, 4096)
    prompt = [(7919 * i + 13) % m.n_vocab for i in range(n_prompt)]
    rates = ([], [])
    runs = 0
    try:
        for rep in range(reps + 1):                             # the first pair warms up
            for k in (0, 1):
                setter(bool(k))
                before = counted()
                b.lib().bamd_kv_cache_clear(ctx.h)
                t0 = time.perf_counter()
                for i in range(0, n_prompt, 512):
                    ctx.decode(prompt[i:i + 512], i)
                if rep:
                    rates[k].append(n_prompt / (time.perf_counter() - t0))
                ran = counted() - before
                assert (ran > 0) == bool(k), "the switch did not select the kernel"
                runs += ran
    finally:
        setter(False)
    assert m.prefill_aux_bytes() == 0
    ctx.close(); m.close()
    return rates[0], rates[1], runs


def print_pair(name, n, path, off, on):
    flop = 2.0 * n * sum(int(t["shape"][0]) * int(t["shape"][1]) for k, t in gguf.GGUFReader(path).tensors.items() if k.startswith("blk.") and len(t["shape"]) == 2)
    bar = max(off) + (max(off) - min(off))
    mo, m1 = statistics.median(off), statistics.median(on)
    print("prompt %-5s %d tokens: switch off median %7.1f tok/s (range %.1f - %.1f; VALU kernel) | switch on median %7.1f tok/s (range %.1f - %.1f; f32 matrix-core kernel, "
          "no side tables) | x %.2f | bar (off max + off spread) %.1f: %s | layer mat-muls %.1f TFLOP per prompt: %.1f TFLOP/s off, %.1f TFLOP/s on = %.1f %% of the f32 MFMA peak"
          % (name, n, mo, min(off), max(off), m1, min(on), max(on), m1 / mo, bar, "cleared" if m1 > bar else "NOT cleared", flop / 1e12, flop * mo / n / 1e12,
             flop * m1 / n / 1e12, 100.0 * flop * m1 / n / MFMA_F32_FLOPS), flush=True)


def measure(name, p, n_prompt, only_prompt=False):
    wb = sum(int(t["data"].size) for n, t in gguf.GGUFReader(p).tensors.items() if len(t["shape"]) == 2 and n != "token_embd.weight")      # what Model.weight_bytes counts
    if not only_prompt:
        r = decode_rate(p)
        med = statistics.median(r)
        print("decode %-5s %6.2f GB file, %6.2f GB of matrices per token: median %7.1f tok/s  (range %.1f - %.1f, 5 x 128 steps after a 128-token prompt) = %4.1f %% of the 8 TB/s token roofline (%.1f tok/s)"
              % (name, os.path.getsize(p) / 1e9, wb / 1e9, med, min(r), max(r), 100.0 * med * wb / HBM_BYTES_PER_S, HBM_BYTES_PER_S / wb), flush=True)
    if n_prompt and name in ("F16", "F32"):
        off, on, _ = prompt_pair(p, n_prompt)
        print_pair(name, n_prompt, p, off, on)
    elif n_prompt and name == "BF16":
        fb = b.prefill_bf16_fallback_tiles()
        off, on, runs = prompt_pair(p, n_prompt, setter=b.set_prefill_bf16, types=(30,))
        print_pair(name, n_prompt, p, off, on)
        print("prompt BF16  %d matrix-core launches while on, %d of their workgroups took the two-rounding VALU step" % (runs, b.prefill_bf16_fallback_tiles() - fb), flush=True)
    elif n_prompt:
        r, aux = prompt_rate(p, n_prompt, reps=5)
        print("prompt %-5s %d tokens: median %7.1f tok/s  (range %.1f - %.1f; %s)" % (name, n_prompt, statistics.median(r), min(r), max(r),
              "VALU kernel" if name != "Q8_0" else "integer-dot kernel"), flush=True)


def main():
    n_prompt = int(sys.argv[sys.argv.index("--prompt") + 1]) if "--prompt" in sys.argv else 0
    types = sys.argv[sys.argv.index("--types") + 1].split(",") if "--types" in sys.argv else ["f16", "bf16", "f32"]
    only_prompt = "--only-prompt" in sys.argv
    if not only_prompt:
        measure("Q8_0", legacy.ensure_model("8b_q8_0"), n_prompt)
    for name in types:
        had = os.path.exists(os.path.join("/dev/shm", "bamd_float_8b_%s.gguf.done" % name))
        p = float_file(name)
        try:
            measure(name.upper(), p, n_prompt, only_prompt)
        finally:
            if not had and "--keep" not in sys.argv:
                os.remove(p); os.remove(p + ".done")


if __name__ == "__main__":
    main()
