"""Greedy decode rate of a synthetic Mixtral-8x7B-shaped file (E 4096, F 14336, L 32, 8 experts, 2 used, the 8-expert Q4_K_M recipe: about 26 GB, written
with reuse_layers=True) beside the dense Llama-3-8B Q4_K_M file, in one job on one card; the time per launch kind of a decode step, the three routed launches
among them; and the share of the token roofline, counting as the bytes of a token the matrices a token streams: every non-expert matrix and the TWO active
experts of every layer, not the eight the file holds.  GPU box only.  Decode: per file a 128-token prompt, then generate_greedy of 128 steps, five repetitions
after a warm-up — median and range.  Launch kinds: bamd_profile_step_kinds (event pairs around every launch of an eager step, the empty pair subtracted), five
steps after a warm-up, medians.  The router and the routed gate/up share kind 4 there; the split of the three routed launches comes from a run of its own
under the profiler's kernel trace (--only-moe --steps-only: eager steps only, every launch a kernel of a stable name).

--recipe NAME[,NAME..]: the same shape under other 8-expert recipes, one after another in this process: q4_k_m (the default), and q4_0, q5_0, q8_0, q4_1, q5_1,
iq4_nl (gguf.mixtral_b32_type: experts of the 32-weight block formats, the routed launches of bamd_moe_b32.h; the Q8_0 file is about 50 GB), and q3_k_m, q2_k,
iq4_xs (the same function over the dense K-quant recipes: Q3_K / Q2_K / IQ4_XS gate and up experts, Q4_K / Q3_K / Q5_K and IQ4_XS down experts).

    python tools/moe_decode.py [--only-moe] [--steps-only] [--recipe q4_k_m,q4_0,q8_0]
"""
import importlib.util
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import booster_amd as b  # noqa: E402
from booster_amd import gguf  # noqa: E402
from lowbit_decode import decode_rate, q4_k_m_file  # noqa: E402

_spec = importlib.util.spec_from_file_location("gen_moe_fixtures", os.path.join(ROOT, "tests", "golden", "gen_moe_fixtures.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
# a model only: no fixture of it is stored
gen.CONFIGS["8x7b"] = (dict(E=4096, H=32, Hkv=8, L=32, F=14336, V=32000, theta=1000000.0), dict(n_expert=8, n_expert_used=2), "mixtral", 128, 128, 512)

SHAPE_8X7B = gen.CONFIGS["8x7b"][0]
_spec = importlib.util.spec_from_file_location("gen_moe_b32_fixtures", os.path.join(ROOT, "tests", "golden", "gen_moe_b32_fixtures.py"))
gen32 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen32)
B32_RECIPES = {"q4_0": gguf.q4_0_type, "q5_0": gguf.q5_0_type, "q8_0": gguf.q8_0_type, "q4_1": gguf.q4_1_type, "q5_1": gguf.q5_1_type, "iq4_nl": gguf.iq4_nl_type}
B32_RECIPES.update({"q3_k_m": gguf.q3_k_m_type, "q2_k": gguf.q2_k_type, "iq4_xs": gguf.iq4_xs_type})      # (K-quant experts through the same 8-expert rules)
for _r, _fn in B32_RECIPES.items():
    gen32.CONFIGS["8x7b_" + _r] = (SHAPE_8X7B, dict(n_expert=8, n_expert_used=2), _fn, 128, 128, 512)


def recipes():
    """the names behind --recipe, in order (default: q4_k_m)"""
    names = sys.argv[sys.argv.index("--recipe") + 1].lower().split(",") if "--recipe" in sys.argv else ["q4_k_m"]
    for r in names:
        if r != "q4_k_m" and r not in B32_RECIPES:
            raise SystemExit("--recipe: %s is none of q4_k_m, %s" % (r, ", ".join(B32_RECIPES)))
    return names


def model_of(recipe):
    """the 8x7B-shaped file under `recipe`, written on first use"""
    return gen.ensure_model("8x7b") if recipe == "q4_k_m" else gen32.ensure_model("8x7b_" + recipe)


HBM_BYTES_PER_S = 8.0e12                                       # MI355X: 8 TB/s
KINDS = ["qkv", "attention", "other", "wo", "router + routed gate/up", "routed down + combine", "lm_head"]


def streamed_bytes(path):
    """(all matrix bytes, the matrix bytes one token streams, n_expert): everything bamd_model_weight_bytes counts, the expert tensors at
    llama.expert_used_count / llama.expert_count of their size"""
    r = gguf.GGUFReader(path)
    n_expert, n_used = int(r.kv.get("llama.expert_count", 0)), int(r.kv.get("llama.expert_used_count", 0))
    n, used = 0, 0
    for name, t in r.tensors.items():
        if not (name.startswith("output.") or ("blk." in name and "norm" not in name)):
            continue
        sz = t["data"].size
        n += sz
        used += sz * n_used // n_expert if "_exps." in name else sz
    return n, used, n_expert


def step_kinds(path, n_prompt=128, reps=5):
    """median over `reps` eager steps (after one warm-up step) of the time per launch kind, the launches and bytes per kind, and the model's layer count"""
    m = b.Model(path)
    n_layer = m.n_layer
    ctx = b.Context(m, 512)
    ctx.decode([(7919 * i + 13) % m.n_vocab for i in range(n_prompt)], 0)
    rows = []
    for rep in range(reps + 1):
        launches, ms, nbytes = ctx.profile_step_kinds(n_prompt + rep)
        rows.append(ms.copy())
    ctx.close(); m.close()
    med = [statistics.median(r[k] for r in rows[1:]) for k in range(8)]
    return launches, med, nbytes, n_layer


def main():
    files = [("Mixtral-8x7B shape, %s" % r.upper(), model_of(r)) for r in recipes()] + ([] if "--only-moe" in sys.argv else [("Llama-3-8B dense, Q4_K_M", q4_k_m_file())])
    for name, p in files:
        total, used, n_expert = streamed_bytes(p)
        print("%-28s file %5.2f GB, matrices %5.2f GB, streamed per token %5.2f GB" % (name, os.path.getsize(p) / 1e9, total / 1e9, used / 1e9), flush=True)
        if "--steps-only" not in sys.argv:
            r = decode_rate(p)
            med = statistics.median(r)
            print("decode %-28s median %7.1f tok/s  (range %.1f - %.1f, 5 x 128 steps after a 128-token prompt) = %.3f of the token roofline (%.2f GB at 8 TB/s = %.1f tok/s)"
                  % (name, med, min(r), max(r), med * used / HBM_BYTES_PER_S, used / 1e9, HBM_BYTES_PER_S / used), flush=True)
        launches, ms, nbytes, n_layer = step_kinds(p)
        for k, kind in enumerate(KINDS):
            if launches[k]:
                us, per_layer = ms[k] * 1e3, max(launches[k] // n_layer, 1)
                print("    %-26s %3d launches, %8.1f us per step = %6.2f us per layer (%d launch%s; eager, event pairs, median of 5 steps), %6.1f MB per layer%s"
                      % (kind if n_expert else kind.replace("router + routed ", "").replace("routed down + combine", "ffn_down"), launches[k], us, us / (launches[k] / per_layer),
                         per_layer, "es" if per_layer > 1 else "", nbytes[k] / (launches[k] / per_layer) / 1e6, " = %.2f TB/s" % (nbytes[k] / (us * 1e-6) / 1e12) if nbytes[k] else ""), flush=True)


if __name__ == "__main__":
    main()
