"""Only the batched prefill (MFMA path), a few repetitions — target for rocprofv3 --kernel-trace --stats (GPU box only).

    python tools/prefill_profile.py [tokens] [8b_q3_k_m | 8b_q2_k]      a low-bit file: with set_prefill_lowbit(True), its prompts on the matrix-core Q3_K / Q2_K kernels
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import booster_amd as b
from booster_amd import gguf
n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
if len(sys.argv) > 2:
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_lowbit_fixtures", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "gen_lowbit_fixtures.py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    path = gen.ensure_model(sys.argv[2])
    b.set_prefill_lowbit(True)
else:
    path = "/dev/shm/bamd_prefill_8b.gguf"
    if not os.path.exists(path):
        gguf.write_synthetic_llama(path, E=4096, H=32, Hkv=8, L=32, F=14336, V=128256, seed=7, reuse_layers=True)
m = b.Model(path); ctx = b.Context(m, 2048 if n <= 2044 else 4096)
toks = [(7919 * i + 13) % 128256 for i in range(n)]
for _ in range(4):
    for i in range(0, n, 512):
        ctx.decode(toks[i:i + 512], i)
