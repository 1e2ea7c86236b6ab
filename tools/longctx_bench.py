"""Prompt and decode rate at long context (BASELINE config 5 shape of the problem): 8B synthetic GGUF, a prompt of n tokens through the batched prefill in
micro-batches of 512, then greedy decode steps with n_kv ~ n (three-kernel attention path).
usage: longctx_bench.py [n_prompt=7936] [n_ctx=8192] [--prompt N] [--n-ctx N] [--scratch-mb MB] [--no-decode]    (GPU box)
  --prompt / --n-ctx   the same two numbers by name; beyond 18 432 positions (e.g. --n-ctx 32768 --prompt 24576) the micro-batches' attention keeps its score rows
                       in the scratch block, and the rate of the micro-batches that END beyond 18 432 is printed on a line of its own
  --scratch-mb MB      budget of that block (bamd_set_attn_scratch_mb; 0 = default)
  --no-decode          the prompt only"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import booster_amd as b
from booster_amd import gguf
argv, opt = [], {}
it = iter(sys.argv[1:])
for a in it:
    if a in ("--prompt", "--n-ctx", "--scratch-mb"):
        opt[a] = int(next(it))
    elif a == "--no-decode":
        opt[a] = 1
    else:
        argv.append(a)
n = opt.get("--prompt", int(argv[0]) if len(argv) > 0 else 7936)
path = "/dev/shm/bamd_prefill_8b.gguf"
if not os.path.exists(path):
    gguf.write_synthetic_llama(path, E=4096, H=32, Hkv=8, L=32, F=14336, V=128256, seed=7, reuse_layers=True)
n_ctx = opt.get("--n-ctx", int(argv[1]) if len(argv) > 1 else 8192)
if "--scratch-mb" in opt and hasattr(b, "set_attn_scratch_mb"):
    b.set_attn_scratch_mb(opt["--scratch-mb"])
m = b.Model(path); ctx = b.Context(m, n_ctx)
toks = [(7919 * i + 13) % 128256 for i in range(n)]
LDS_POSITIONS = 18432                    # two score rows of a sequence fit the LDS up to here
t0 = time.perf_counter(); t_far = n_far = 0
for i in range(0, n, 512):
    t1 = time.perf_counter()
    ctx.decode(toks[i:i + 512], i)       # (returns the logits: synchronous)
    if min(i + 512, n) > LDS_POSITIONS:
        t_far += time.perf_counter() - t1; n_far += min(i + 512, n) - i
tp = time.perf_counter() - t0
print("prefill %d tokens: %.1f ms (%.0f tok/s)" % (n, tp * 1e3, n / tp))
if n_far:
    print("  micro-batches beyond %d positions: %d tokens in %.1f ms (%.0f tok/s); up to there %d tokens in %.1f ms (%.0f tok/s)"
          % (LDS_POSITIONS, n_far, t_far * 1e3, n_far / t_far, n - n_far, (tp - t_far) * 1e3, (n - n_far) / max(tp - t_far, 1e-9)))
if "--no-decode" not in opt:
    ctx.generate_greedy(n, 8)
    out, ms = ctx.generate_greedy(n + 8, 64)
    kvb = 131072 * (n + 40)
    print("decode at n_kv ~ %d: %.3f ms/token = %.1f tok/s; bytes/token %.2f GB -> %.0f GB/s (%.1f %% of 8 TB/s)" % (n + 40, ms / 64, 64e3 / ms, (4.6174e9 + kvb) / 1e9, (4.6174e9 + kvb) / (ms / 64 * 1e-3) / 1e9, (4.6174e9 + kvb) / (ms / 64 * 1e-3) / 8e12 * 100))
