"""Greedy decode rate and prompt rate of the synthetic Llama-3-8B file under the Q8_0, Q4_0 and Q5_0 recipes beside the Q4_K_M file, in one job on one card.
GPU box only.  Decode: per file a 128-token prompt, then generate_greedy of 128 steps, five repetitions after a warm-up; prompt: N tokens in micro-batches of
512, five repetitions after a warm-up (the Q8_0 / Q4_0 / Q5_0 files on the integer-dot kernel: they have no matrix-core kernel) — median and range.

    python tools/legacy_decode.py [--prompt 2048]
"""
import importlib.util
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from booster_amd import gguf  # noqa: E402
from lowbit_decode import decode_rate, prompt_rate, q4_k_m_file  # noqa: E402

_spec = importlib.util.spec_from_file_location("gen_legacy_fixtures", os.path.join(ROOT, "tests", "golden", "gen_legacy_fixtures.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
gen.CONFIGS.setdefault("8b_q5_0", (gen.L3_8B, "q5_0", 128, 64, 512))          # a model only: no fixture of it is stored


def main():
    files = [("Q4_K_M", q4_k_m_file()), ("Q8_0", gen.ensure_model("8b_q8_0")), ("Q4_0", gen.ensure_model("8b_q4_0")), ("Q5_0", gen.ensure_model("8b_q5_0"))]
    for name, p in files:
        r = decode_rate(p)
        print("decode %-7s %5.2f GB: median %7.1f tok/s  (range %.1f - %.1f, 5 x 128 steps after a 128-token prompt)" % (name, os.path.getsize(p) / 1e9, statistics.median(r), min(r), max(r)), flush=True)
    if "--prompt" in sys.argv:
        n = int(sys.argv[sys.argv.index("--prompt") + 1])
        for name, p in files:
            r, aux = prompt_rate(p, n, reps=5)
            print("prompt %-7s %d tokens: median %7.1f tok/s  (range %.1f - %.1f; %s)" % (name, n, statistics.median(r), min(r), max(r),
                  "matrix-core kernels" if aux > 0 else "integer-dot kernel"), flush=True)


if __name__ == "__main__":
    main()
