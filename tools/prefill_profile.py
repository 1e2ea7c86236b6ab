"""Only the batched prefill (MFMA path), a few repetitions — target for rocprofv3 --kernel-trace --stats (GPU box only).

    python tools/prefill_profile.py [tokens] [8b_q3_k_m | 8b_q2_k]      a low-bit file: with set_prefill_lowbit(True), its prompts on the matrix-core Q3_K / Q2_K kernels
    python tools/prefill_profile.py [tokens] [8b_q8_0 | 8b_q4_0 | 8b_q5_0]   a legacy-quant file: with set_prefill_q0(True), its prompts on the Q8_0 / Q4_0 / Q5_0 matrix-core kernel
    python tools/prefill_profile.py [tokens] [8b_q4_1 | 8b_q5_1 | 8b_q4_0_imat]   with set_prefill_q1(True) (8b_q4_0_imat: both switches), on the Q4_1 / Q5_1 matrix-core kernel
    python tools/prefill_profile.py [tokens] 8b_iq4nl                   the IQ4_NL recipe's file: with set_prefill_nl(True), on the IQ4_NL matrix-core kernel
    a trailing "off" leaves the switches off: the same prompts on the integer-dot kernels
"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import booster_amd as b
from booster_amd import gguf
n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
if len(sys.argv) > 2:
    import importlib.util
    legacy = sys.argv[2] in ("8b_q8_0", "8b_q4_0", "8b_q5_0")
    legacy1 = sys.argv[2] in ("8b_q4_1", "8b_q5_1", "8b_q4_0_imat")
    iq4nl = sys.argv[2] == "8b_iq4nl"
    name = "gen_legacy_fixtures" if legacy else "gen_legacy1_fixtures" if legacy1 else "gen_iq4nl_fixtures" if iq4nl else "gen_lowbit_fixtures"
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", name + ".py"))
    gen = importlib.util.module_from_spec(spec); spec.loader.exec_module(gen)
    if legacy:
        gen.CONFIGS.setdefault("8b_q5_0", (gen.L3_8B, "q5_0", 128, 64, 512))          # a model only: no fixture of it is stored
    if legacy1:
        gen.CONFIGS.setdefault(sys.argv[2], (gen.L3_8B, {"8b_q4_1": "q4_1", "8b_q5_1": "q5_1", "8b_q4_0_imat": "q4_0_imatrix"}[sys.argv[2]], 128, 64, 512))
    if iq4nl:
        gen.CONFIGS.setdefault("8b_iq4nl", (dict(E=4096, H=32, Hkv=8, L=32, F=14336, V=128256, theta=500000.0), dict(imatrix=False), False, 128, 64, 512))
    path = gen.ensure_model(sys.argv[2])
    if sys.argv[-1] == "off":
        pass
    elif iq4nl:
        b.set_prefill_nl(True)
    elif legacy1:
        b.set_prefill_q1(True); b.set_prefill_q0(sys.argv[2] == "8b_q4_0_imat")
    else:
        b.set_prefill_q0(True) if legacy else b.set_prefill_lowbit(True)
else:
    path = "/dev/shm/bamd_prefill_8b.gguf"
    if not os.path.exists(path):
        gguf.write_synthetic_llama(path, E=4096, H=32, Hkv=8, L=32, F=14336, V=128256, seed=7, reuse_layers=True)
m = b.Model(path); ctx = b.Context(m, 2048 if n <= 2044 else 4096)
toks = [(7919 * i + 13) % 128256 for i in range(n)]
for _ in range(4):
    for i in range(0, n, 512):
        ctx.decode(toks[i:i + 512], i)
