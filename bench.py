#!/usr/bin/env python3
"""bench.py — decode tokens/s, Llama-3-8B Q4_K_M shapes, greedy batch-1 decode (BASELINE.json configs[1]).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]     (N > 1: launched by torch.distributed.run, one rank per GPU)

One "step" = one decoded token through the whole hot path (32 layers + lm_head + arg-max), weights and KV cache
resident in HBM, token feedback on the device.  Synthetic GGUF with the exact tensor names / shapes / K-quant types
of Llama-3-8B Q4_K_M (random blocks), 128-token prompt, n_ctx 512.

N = 1: the whole model on one GPU, K steps replayed from one hipGraph per step.
N > 1: Booster's `gpus:` layer split (llama.cpp:5932-5969), one process per GPU: rank r owns a contiguous layer
       range, its KV slice, (rank 0) the embedding, (last rank) output_norm + lm_head.  The f32 hidden state
       [n_embd] moves with ONE RCCL send/recv per boundary (torch.distributed, backend nccl = RCCL over xGMI); the
       arg-max token returns from the last rank to rank 0 with one more send/recv.  `value` stays the BASELINE
       metric — batch-1 decode of ONE sequence, now through N stages that work one after another (total work fixed:
       "strong"); the throughput with N independent sequences in flight (Booster's pods) is reported beside it.
--model 70b: the same with Llama-3-70B Q4_K_M shapes (80 layers; BASELINE config 4 at --gpus 8); m7q6k: Mistral-7B, all Q6_K.

Prints ONE JSON line (rank 0).  At N = 1 a plain run sets up, runs W warm-up steps, times EXACTLY K steps in one window (`value`, `ms_per_step`),
writes --dump-outputs and prints the line.  --dump-outputs DIR: what that timed call returned, DIR/tokens.npy (the K + 1 tokens of
Context.generate_greedy, as float64) and DIR/logits.npy (the last step's logits, float32); the inputs are seeded, so the same arguments give the same inputs.
--full adds everything below, measured after the headline window: `config.repeats` (four more windows of the same K steps), the prompt rate, `roofline`,
`config.secondary` and `cpu_baseline`.  `roofline` is for the DOMINANT kernel — the launch kind with the largest share of the step time
(gate/up on this workload): achieved = its algorithmic weight bytes per launch / its mean launch duration, measured here with HIP
events around every launch of eager steps; `roofline.per_kind` lists every launch kind the same way and
`roofline.all_matvec_launches` the average over all weight-streaming launches (the figure round 1 reported); `traffic` is NOT measured in this run: it is the per-launch HBM read bytes of the committed
rocprofv3 PMC pass (profiles/), quoted for comparison.  `cpu_baseline` times the GENUINE reference CPU path
(oracle/_ref/ref_bench, built in the build container and shipped prebuilt) on this box's host cores on the same GGUF:
a 16-token prefill and 64 single-token decode steps per point of a thread / placement sweep, rank 0, N = 1 only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CFG_8B = dict(E=4096, H=32, Hkv=8, L=32, F=14336, V=128256, theta=500000.0, eps=1e-5, n_ctx_train=8192)
CFG_70B = dict(E=8192, H=64, Hkv=8, L=80, F=28672, V=128256, theta=500000.0, eps=1e-5, n_ctx_train=8192)
CFG_M7 = dict(E=4096, H=32, Hkv=8, L=32, F=14336, V=32000, theta=10000.0, eps=1e-5, n_ctx_train=8192)
MODELS = {"8b": ("Llama-3-8B Q4_K_M", CFG_8B, "bamd_llama3_8b_q4_k_m_synth.gguf"),
          "70b": ("Llama-3-70B Q4_K_M", CFG_70B, "bamd_llama3_70b_q4_k_m_synth.gguf"),
          "m7q6k": ("Mistral-7B Q6_K", CFG_M7, "bamd_mistral7b_q6_k_synth.gguf")}
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec (MI355X_MICROARCH.md); measured copy ceiling 6290 GB/s
N_PROMPT, N_CTX = 128, 512
from booster_amd.pipeline import SCALING_NOTE  # noqa: E402  (host-side text only)
KV_BYTES_PER_POS = 2 * 32 * 8 * 128 * 2


def model_path(model="8b"):
    name = MODELS[model][2]
    need = (48 << 30) if model == "70b" else (7 << 30)
    for d in ("/dev/shm", "/tmp"):
        if os.path.isdir(d) and os.access(d, os.W_OK):
            try:
                if os.path.exists(os.path.join(d, name + ".done")):
                    return os.path.join(d, name)
                st = os.statvfs(d)
                if st.f_bavail * st.f_frsize > need:
                    return os.path.join(d, name)
            except OSError:
                pass
    return os.path.join("/tmp", name)


def ensure_model(path, rank, model="8b"):
    from booster_amd import gguf
    done = path + ".done"
    if rank == 0 and not os.path.exists(done):
        t0 = time.time()
        kw = dict(MODELS[model][1])
        if model == "70b":
            kw["type_fn"] = lambda name, il: gguf.q4_k_m_type_70b(name, il, 80)
        elif model == "m7q6k":
            kw["type_fn"] = lambda name, il: gguf.Q6_K
            kw["embd_type"] = gguf.Q6_K
        gguf.write_synthetic_llama(path, seed=7, reuse_layers=True, **kw)
        open(done, "w").write("ok")
        sys.stderr.write("[bench] wrote %s (%.1f GB) in %.1f s\n" % (path, os.path.getsize(path) / 1e9, time.time() - t0))
    return path


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def physical_cores(limit):
    """physical cores this process may run on: distinct (package, core) pairs of /proc/cpuinfo among the CPUs of the affinity mask"""
    try:
        allowed = os.sched_getaffinity(0)
    except AttributeError:
        allowed = None
    seen, cpu, pkg = set(), None, None
    try:
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k = k.strip()
            if k == "processor":
                cpu = int(v)
            elif k == "physical id":
                pkg = int(v)
            elif k == "core id" and (allowed is None or cpu in allowed):
                seen.add((pkg, int(v)))
    except (OSError, ValueError):
        pass
    return max(1, min(len(seen) or limit, limit))


def split_layers(L, n):
    """Booster's gpus: semantic with equal weights (llama.cpp:5954-5958: upper_bound over the cumulative split)."""
    cuts = [int(round(L * (i + 1) / n)) for i in range(n)]
    first = [0] + cuts[:-1]
    return list(zip(first, cuts))


def socket0_cpus():
    """logical CPUs of physical package 0 that this process may use, one per core first (SMT siblings last): where a pinned run of the reference is placed"""
    try:
        allowed = os.sched_getaffinity(0)
    except AttributeError:
        return []
    first, rest, seen, cpu, pkg = [], [], set(), None, None
    try:
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k = k.strip()
            if k == "processor":
                cpu = int(v)
            elif k == "physical id":
                pkg = int(v)
            elif k == "core id" and pkg == 0 and cpu in allowed:
                (rest if int(v) in seen else first).append(cpu); seen.add(int(v))
    except (OSError, ValueError):
        pass
    return first + rest


def cpu_baseline_reference(path, nthreads, pinned=False, n_decode=64):
    """The GENUINE reference CPU path (oracle/_ref/ref_bench: ggml + llama.cpp of gotzmann/booster compiled in place by
    oracle/Makefile with Booster's `make cpu` flags, -march=x86-64-v3) on the same GGUF, all 32 layers: a 16-token prefill and
    n_decode single-token llama_decode steps; the metric is the reference's own t_eval definition (llama.cpp:18527-18551).
    pinned: OMP_PROC_BIND=close OMP_PLACES=cores, under numactl --cpunodebind=0 --membind=0 where numactl exists, else with the
    affinity mask cut to the cores of package 0 (when they suffice).  None if the binary is not there."""
    import re
    import shutil
    import subprocess
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_bench")
    if not os.path.exists(exe):
        return None
    n_prompt = 16
    env = dict(os.environ, OMP_NUM_THREADS=str(nthreads))
    cmd, pre, how = [exe, path, str(nthreads), str(n_prompt), str(n_decode), "512"], None, "unpinned"
    if pinned:
        env.update(OMP_PROC_BIND="close", OMP_PLACES="cores")
        how = "OMP_PROC_BIND=close OMP_PLACES=cores"
        s0 = socket0_cpus()
        if shutil.which("numactl") and len(s0) >= nthreads:
            cmd = ["numactl", "--cpunodebind=0", "--membind=0"] + cmd; how += ", numactl --cpunodebind=0 --membind=0"
        elif len(s0) >= nthreads:
            pre = lambda: os.sched_setaffinity(0, set(s0))
            how += ", affinity = the %d CPUs of package 0" % len(s0)
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=600, env=env, check=True, preexec_fn=pre).stdout.decode()
    m = re.search(r"tokens_per_s=([0-9.]+) ms_per_token=([0-9.]+) prompt_tokens_per_s=([0-9.]+)", out)
    return dict(value=round(float(m.group(1)), 4), unit="tokens/s", cores=nthreads, kind="reference", placement=how,
                sample="genuine reference CPU path (gotzmann/booster's ggml + llama.cpp built by oracle/Makefile, `make cpu` flags with -march=x86-64-v3) "
                       "on %d threads (%s) of this box's host (%s, %d logical CPUs) on the same GGUF, all layers: %d-token prefill (%.1f tok/s) + %d greedy "
                       "single-token llama_decode steps, %.1f ms per token.  Build-container figures for config 1 (128 + 128 tokens, threads = 1 and 8): BASELINE.md section 3"
                       % (nthreads, how, cpu_name(), os.cpu_count() or 0, n_prompt, float(m.group(3)), n_decode, float(m.group(2))))


def cpu_baseline(path, nthreads):
    """Fallback when oracle/_ref is absent: the oracle (port of the reference CPU path) on a bounded sample: decode steps through
    the first 1 and 2 layers + lm_head, extrapolated to 32 layers.  Checker code only — never part of the measured GPU path."""
    from oracle import pyoracle as po
    from booster_amd.gguf import GGUFReader
    r = GGUFReader(path)
    times = {}
    for nl in (1, 2):
        m = po.OracleModel(r, n_layers=nl)
        c = po.OracleContext(m, 64, nthreads=nthreads)
        c.decode([13], 0)                                 # touch pages / warm caches
        t0 = time.perf_counter()
        reps = 3
        for i in range(reps):
            c.decode([(7919 * i + 13) % CFG_8B["V"]], 1 + i)
        times[nl] = (time.perf_counter() - t0) / reps
        c.close()
    per_layer = max(times[2] - times[1], 1e-9)
    head = max(times[1] - per_layer, 0.0)
    t_tok = head + CFG_8B["L"] * per_layer
    return dict(value=round(1.0 / t_tok, 4), unit="tokens/s", cores=nthreads, kind="port",
                sample="oracle (C restatement of the reference CPU path, %d OpenMP threads): 3 decode steps each through 1 and 2 of 32 "
                       "layers + lm_head of the same GGUF; per-layer %.1f ms, lm_head+embed %.1f ms, extrapolated to 32 layers"
                       % (nthreads, per_layer * 1e3, head * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--full", action="store_true", help="N = 1: after the headline window, also measure config.repeats, the prompt rate, the per-kind roofline, "
                                                        "the secondary configurations and the CPU baseline (a plain run times the K steps and nothing else)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="N = 1: write what the last timed call returned (tokens, last step's logits) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--model", default="8b", choices=sorted(MODELS), help="8b = the BASELINE metric (default); 70b = BASELINE config 4 shapes; m7q6k = config 5 shapes")
    ap.add_argument("--pipeline-smoke", action="store_true", help="run the N > 1 code path (layer-split pipeline, RCCL group) with a single rank")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="gloo: CPU plumbing check of the N > 1 leg (launch, rendezvous, schedule, JSON) "
                                                                               "with a stand-in stage — tests/test_bench_selflaunch.py; never a measurement")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the secondary configurations (BASELINE configs 3, 5 and 4 at N = 1) of the N = 1 line")
    args = ap.parse_args()
    N = args.gpus
    if args.dump_outputs and (N > 1 or args.pipeline_smoke or args.backend == "gloo"):
        ap.error("--dump-outputs is for the N = 1 line")
    if N > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` as the N = 1 line is started: no launcher given, so be the launcher — one rank per GPU under
        # torch.distributed.run on this node (the reference's split needs none either: one process, cpp/bridge.cpp:745-750)
        sys.exit(self_launch(N, sys.argv[1:]))
    rank = int(os.environ.get("RANK", "0")); world = int(os.environ.get("WORLD_SIZE", "1")); local = int(os.environ.get("LOCAL_RANK", "0"))
    import torch
    dist = None
    if args.backend == "gloo":
        import torch.distributed as dist
        assert world == N, "WORLD_SIZE %d but --gpus %d" % (world, N)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29517")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from booster_amd import pipeline
        result = pipeline.run_plumbing_check(N, rank, [3, 1, 4, 1, 5], args.warmup, args.steps, dist, pipeline.FakeStage)
        emit(rank, dist, result, "plumbing check (stand-in stage, vocabulary %d)" % pipeline.FakeStage.V, N, args.steps, args.warmup)
        return
    import booster_amd
    from booster_amd import build as bbuild
    if rank == 0:
        bbuild.build()
    if N > 1 or args.pipeline_smoke:
        import torch.distributed as dist
        assert world == N, "WORLD_SIZE %d but --gpus %d (bench.py launches its own ranks when WORLD_SIZE is absent)" % (world, N)
        torch.cuda.set_device(local)
        if "MASTER_ADDR" not in os.environ:
            os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ.setdefault("MASTER_PORT", "29517")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
    model_name, CFG, _ = MODELS[args.model]
    path = model_path(args.model)
    if dist is not None:                                  # rank 0 picks the directory (free space changes while it writes): every rank uses its choice
        box = [path]
        dist.broadcast_object_list(box, src=0)
        path = box[0]
    ensure_model(path, rank, args.model)
    if dist is not None:
        dist.barrier()
    steps, warmup = args.steps, args.warmup
    # the default K / W fit the 512-position context the metric is quoted on; a longer request grows the context instead of failing
    n_ctx = max(N_CTX, (N_PROMPT + warmup + steps + 2 + 255) // 256 * 256)
    prompt = [(7919 * i + 13) % CFG["V"] for i in range(N_PROMPT)]
    result = {}

    if N == 1 and not args.pipeline_smoke:
        t0 = time.time()
        m = booster_amd.Model(path, device=0)
        ctx = booster_amd.Context(m, n_ctx)
        sys.stderr.write("[bench] model resident: %.3f GB of matmul weights, load %.1f s\n" % (m.weight_bytes / 1e9, time.time() - t0))
        ctx.decode(prompt[:8], 0)                                          # allocate the batched-prefill buffers
        tp0 = time.perf_counter()
        ctx.decode(prompt, 0)                                              # prefill: one micro-batch through the batched kernels (not part of `value`)
        prefill_tok_s = len(prompt) / (time.perf_counter() - tp0)
        n_past = N_PROMPT
        if warmup > 0:
            ctx.generate_greedy(n_past, warmup); n_past += warmup
        # The timed region: EXACTLY K steps between two synchronisations; `value` and `ms_per_step` are this one window
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks, ev_ms = ctx.generate_greedy(n_past, steps)                   # K replays of the step, no host round trips
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, tokens=toks, logits=ctx.last_logits())
        tok_s = steps / dt
        n_kv_avg = N_PROMPT + warmup + steps / 2.0
        kv_bytes_per_pos = 2 * CFG["L"] * CFG["Hkv"] * (CFG["E"] // CFG["H"]) * 2
        bytes_per_token = m.weight_bytes + kv_bytes_per_pos * n_kv_avg
        result = dict(
            value=round(tok_s, 2), ms_per_step=round(dt / steps * 1e3, 4), scaling="strong",      # the same word on every line: one sequence, total work fixed as N grows (config.scaling_note)
            config=dict(workload="%s shapes (synthetic GGUF, random K-quant blocks), greedy batch-1 decode on 1xMI355X, "
                                 "128-token prompt, n_ctx %d, n_kv %d..%d" % (model_name, n_ctx, N_PROMPT + warmup, n_past + steps),
                        parallelism="single GPU", scaling_note=SCALING_NOTE,
                        aql_runs=ctx.aql_runs(), replay=("AQL packets, fence scope NONE, own HSA queue (csrc/bamd_aql.h)" if ctx.aql_runs() > 0 else "one hipGraph per step on a HIP stream"), graph_event_ms_per_step=round(ev_ms / steps, 4),
                        bytes_per_token=int(bytes_per_token), frac_of_hbm_roofline_tokens=round(tok_s * bytes_per_token / (HBM_PEAK_GBS * 1e9), 4)))
        if args.full:
            full_measurements(args, result, booster_amd, m, ctx, torch, CFG, n_past, steps, dt, prefill_tok_s, bytes_per_token, path)
        ctx.close(); m.close()
    else:
        from booster_amd import pipeline
        result = pipeline.run_layer_split_bench(path, CFG, N, rank, local, prompt, n_ctx, warmup, steps, dist, torch, model_name)

    emit(rank, dist, result, model_name, N, steps, warmup)


def dump_outputs(d, **arrays):
    """--dump-outputs: what the timed call returned, as <d>/<name>.npy (integers as float64, which holds every int32 exactly; floats as float32)"""
    os.makedirs(d, exist_ok=True)
    for name, a in arrays.items():
        a = np.asarray(a)
        np.save(os.path.join(d, name + ".npy"), a.astype(np.float64 if a.dtype.kind in "iu" else np.float32))


def full_measurements(args, result, booster_amd, m, ctx, torch, CFG, n_past, steps, dt, prefill_tok_s, bytes_per_token, path):
    """--full: everything beyond the headline window, added to `result` — four more windows of the same K steps (config.repeats), the prompt
    evaluation rate, the roofline of every launch kind from eager steps, the secondary configurations and the CPU baseline"""
    # Four more windows of EXACTLY K steps, back to back over the SAME positions as the headline window (the K steps rewrite the same KV rows, so every
    # repetition is the metric's n_kv range); config.repeats carries min / median / max over all five (one window alone is at the mercy of whatever else
    # the box does in those milliseconds)
    reps_dt = [dt]
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.generate_greedy(n_past, steps)
        torch.cuda.synchronize()
        reps_dt.append(time.perf_counter() - t0)
    n_past += steps
    tok_s = steps / dt
    repeats = dict(n=5, tokens_per_s=dict(min=round(steps / max(reps_dt), 2), median=round(steps / sorted(reps_dt)[2], 2), max=round(steps / min(reps_dt), 2)),
                   note="same K steps over the same positions, back to back; value = the first repetition (the headline window)")
    # roofline of the dominant kernel: HIP events around every launch of eager steps at the same context length, per launch kind
    KINDS = ["qkv", "attention", "other", "wo", "gate_up", "ffn_down", "lm_head"]
    KERNEL_OF = {"qkv": "matvec_split_mixed_kernel (fused QKV, RMSNorm prologue, three row-groups per workgroup in one batch)", "wo": "matvec_split_fast_kernel (wo, +residual)",
                 "gate_up": "matvec_gateup7_kernel<12, 2> at the 8B / Mistral widths (seven row-group pairs per workgroup; matvec_gateup14_kernel at the 70B widths, matvec_fast_kernel<TYPE, 0, RMSNorm prologue, silu(gate)*up epilogue> elsewhere): ffn_gate + ffn_up of one layer in one launch", "ffn_down": "matvec_split_fast_kernel (ffn_down, +residual)",
                 "lm_head": "matvec_fast_kernel<Q6_K, arg-max epilogue> (output)", "attention": "attn_fused_kernel",
                 "attention+wo": "attn_wo_kernel (single-launch attention on H CUs, wo + residual on the others)"}
    # eight eager steps; per launch kind the MEDIAN step's time (one eager step that catches a clock ramp or a neighbour's burst would otherwise move a kind's
    # share by 10-15 %: the round-5 profile run read gate/up at 15.5 us once against 13.5-13.7 in every other run)
    ev_over = []
    reps = 8
    per_rep = []
    for i in range(reps):
        l, ms, b = ctx.profile_step_kinds(n_past - 1)
        per_rep.append((np.array(l[:7], float), np.array(ms[:7], float), np.array(b[:7], float))); ev_over.append(ms[7])
    LK = per_rep[0][0] * reps; BK = per_rep[0][2] * reps                   # launches and bytes per kind are the same in every step
    MSK = np.median(np.stack([r[1] for r in per_rep]), axis=0) * reps
    mv = [0, 3, 4, 5, 6]                                             # the mat-vec launches; 1 = attention, 2 = other
    L_ = np.array([LK[mv].sum(), LK[1], LK[2]]); MS_ = np.array([MSK[mv].sum(), MSK[1], MSK[2]]); B_ = np.array([BK[mv].sum(), BK[1], BK[2]])
    ev_empty_ms = float(np.median(ev_over))                          # what an EMPTY event pair reads on the same stream
    # An event pair around a kernel adds less than an empty pair reads (the second record overlaps the kernel's tail), so the
    # per-launch overhead is calibrated against the timed region itself: the eager per-launch times of one step, minus the
    # overhead, must add up to the step time the hipGraph replay measured above.  (Check: rocprofv3's mean durations
    # for the same workload, profiles/r02_kernel_stats.csv.)
    step_ms = dt / steps * 1e3
    ev_overhead_ms = min(max((float(MS_.sum()) / reps - step_ms) / (float(L_.sum()) / reps), 0.0), ev_empty_ms)
    mv_bytes_per_launch = B_[0] / L_[0]
    mv_ms_per_launch = max(MS_[0] / L_[0] - ev_overhead_ms, 1e-6)
    family_achieved = mv_bytes_per_launch / (mv_ms_per_launch * 1e-3) / 1e9
    # the DOMINANT kernel = the launch kind with the largest share of the step time
    per_kind = {}
    for k in range(7):
        if LK[k] > 0:
            t_ms = max(MSK[k] / LK[k] - ev_overhead_ms, 1e-6)
            per_kind[KINDS[k]] = dict(launches_per_token=int(LK[k] / reps), us_per_launch=round(t_ms * 1e3, 3), bytes_per_launch=int(BK[k] / LK[k]),
                                      GBps=round(BK[k] / LK[k] / (t_ms * 1e-3) / 1e9, 1), share_of_step=round(t_ms * LK[k] / reps / step_ms, 4))
    if "wo" not in per_kind and "attention" in per_kind:             # attention and wo share a launch (bamd_colaunch.hip): its bytes are wo's weights
        per_kind = {("attention+wo" if k == "attention" else k): v for k, v in per_kind.items()}
    dom = max((k for k in per_kind if k not in ("other",)), key=lambda k: per_kind[k]["share_of_step"])
    achieved = per_kind[dom]["GBps"]
    # HBM bytes per launch of the dominant kernel, quoted from the NEWEST committed rocprofv3 PMC pass of this workload (profiles/r*_pmc_fetch_summary.json:
    # FETCH_SIZE in its own pass, x 1024 x 2 per MI355X_MICROARCH.md).  The kernel is found by what it reads, not by a hard-coded template name: the
    # mat-vec entry whose mean traffic is closest to this launch kind's algorithmic bytes, and it must lie within [0.95, 1.25] x those bytes — anything
    # else means the summary is of another workload / kernel set, and the field stays null with the reason beside it.
    traffic, traffic_source = None, None
    try:
        if args.model == "8b":
            import glob
            cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_fetch_summary.json")))
            if cands:
                pm = json.load(open(cands[-1]))
                want = per_kind[dom]["bytes_per_launch"]
                mvk = {k: v["mean_hbm_read_bytes"] for k, v in pm["per_kernel"].items() if k.startswith("matvec")}
                best = min(mvk, key=lambda k: abs(mvk[k] - want)) if mvk else None
                if best is not None and 0.95 * want <= mvk[best] <= 1.25 * want:
                    traffic = int(mvk[best])
                    traffic_source = "profiles/%s, kernel %s (committed rocprofv3 --pmc FETCH_SIZE pass of this workload; not measured in this run)" % (os.path.basename(cands[-1]), best)
                else:
                    traffic_source = "no mat-vec kernel in profiles/%s reads within [0.95, 1.25] x %d B per launch (closest: %s = %s B)" % (os.path.basename(cands[-1]), want, best, mvk.get(best))
                    sys.stderr.write("[bench] roofline.traffic left null: " + traffic_source + "\n")
    except Exception as e:
        traffic_source = "failed to read the committed PMC summary: %r" % (e,)
        sys.stderr.write("[bench] roofline.traffic left null: " + traffic_source + "\n")
    result["config"].update(
        repeats=repeats,
        time_split_ms_per_token=dict(matvec=round(MS_[0] / reps - L_[0] / reps * ev_overhead_ms, 4), attention=round(MS_[1] / reps - L_[1] / reps * ev_overhead_ms, 4),
                                     other=round(max(MS_[2] / reps - L_[2] / reps * ev_overhead_ms, 0.0), 4)),
        prompt_eval_tokens_per_s=round(prefill_tok_s, 1), launches_per_token=int((L_[0] + L_[1] + L_[2]) / reps), event_pair_overhead_us=round(ev_overhead_ms * 1e3, 3), empty_event_pair_us=round(ev_empty_ms * 1e3, 3))
    result["roofline"] = dict(bound="hbm", achieved=round(achieved, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(achieved / HBM_PEAK_GBS, 4),
                              # the WHOLE step against the roofline (every byte a token needs / the step time), beside the dominant kernel's own fraction
                              step_frac=round(tok_s * bytes_per_token / (HBM_PEAK_GBS * 1e9), 4), step_achieved=round(tok_s * bytes_per_token / 1e9, 1),
                              # HBM bytes are NOT counted in this run (PMC counters need their own rocprofv3 pass): null here; the committed pass is quoted beside it
                              traffic=None, traffic_committed_pmc=traffic, traffic_source=traffic_source,
                              kernel="%s: %s — the launch kind with the largest share of the step (%.1f %%)" % (dom, KERNEL_OF.get(dom, dom), 100.0 * per_kind[dom]["share_of_step"]),
                              bytes_per_launch=per_kind[dom]["bytes_per_launch"], us_per_launch=per_kind[dom]["us_per_launch"],
                              per_kind=per_kind,
                              all_matvec_launches=dict(GBps=round(family_achieved, 1), frac=round(family_achieved / HBM_PEAK_GBS, 4), bytes_per_launch=int(mv_bytes_per_launch),
                                                       us_per_launch=round(mv_ms_per_launch * 1e3, 3)))
    if not args.no_secondary and args.model == "8b":
        result["config"]["secondary"] = secondary_configs(booster_amd, m, torch)
    if not args.no_cpu_baseline:
        try:
            try:
                ncpu = len(os.sched_getaffinity(0))
            except AttributeError:
                ncpu = os.cpu_count() or 1
            omp = os.environ.get("OMP_NUM_THREADS", "").split(",")[0]
            if omp.isdigit() and int(omp) > 0:
                ncpu = min(ncpu, int(omp))                                   # where the environment sets the CPUs this run may use, no sweep point goes beyond them
            phys = physical_cores(ncpu)
            # the reference's best on this box: its OpenMP decode is memory- and barrier-bound and gets SLOWER beyond one socket's worth of
            # threads, so the sweep covers {8, 16, 24, 32, 48} each unpinned and pinned to cores of one package, plus 12 and 20 unpinned around the optimum measured in round 6;
            # 64 decode steps per point (~3-8 s each, bounded by `budget`); the best point is the baseline, the whole sweep rides along
            cands = sorted(set(max(1, min(ncpu, c)) for c in (8, 12, 16, 20, 24, 32, 48) if c <= max(phys, 8)))
            ref, sweep, t_sweep, budget = None, {}, time.time(), 150.0
            try:
                for c in sorted(cands, key=lambda c: abs(c - 18)):           # the likely optimum first (round 6, 2 x EPYC 9575F: 16 threads unpinned 34.9 tok/s, 32: 19.6): a box that runs out of budget still has it
                    for pinned in ((False,) if c in (12, 20) else (False, True)):
                        if time.time() - t_sweep > budget:
                            sweep["%d%s" % (c, "p" if pinned else "")] = "skipped (sweep budget)"
                            continue
                        r = cpu_baseline_reference(path, c, pinned)
                        if r is None:
                            break
                        sweep["%d%s" % (c, "p" if pinned else "")] = r["value"]
                        if ref is None or r["value"] > ref["value"]:
                            ref = r
                if ref is not None:
                    ref["thread_sweep_tokens_per_s"] = dict(points=sweep, key="<threads>[p = pinned: OMP_PROC_BIND=close OMP_PLACES=cores on package 0]",
                                                            seconds=round(time.time() - t_sweep, 1))
                    ref["physical_cores"] = phys
            except Exception as e:
                sys.stderr.write("[bench] reference cpu baseline failed (%r); falling back to the oracle port\n" % (e,))
                ref = None
            result["cpu_baseline"] = ref if ref is not None else cpu_baseline(path, max(1, min(ncpu, 32)))
        except Exception as e:      # the checker must never take the bench down
            result["cpu_baseline"] = dict(value=None, unit="tokens/s", cores=0, kind="port", sample="failed: %r" % (e,))


def secondary_configs(booster_amd, m8b, torch):
    """BASELINE.json's other single-GPU configurations, measured in the same run and reported under config.secondary (bounded: ~1 min in all; each
    leg is skipped with its reason rather than taking the line down):
      config3     Llama-3-8B Q4_K_M, 2048-token prompt in micro-batches of 512 at n_ctx 4096: tokens/s, TFLOP/s of mat-mul work, fraction of the dense f16 MFMA peak
      config5     Mistral-7B shape, every matrix Q6_K, n_ctx 8192: decode at ~8000 cached positions THROUGH THE BRIDGE (the nine cgo symbols, Janus sampling
                  with the device prefilter): tokens/s and the fraction of that shape's token roofline
      config4_n1  the whole Llama-3-70B Q4_K_M on ONE GPU (the N = 1 point of the layer split), when /dev/shm has room for its 42 GB file"""
    sec = {}
    t_all = time.time()
    try:                                                                   # ---- config 3
        V = CFG_8B["V"]; n = 2048
        toks = [(7919 * i + 13) % V for i in range(n)]
        ctx = booster_amd.Context(m8b, 4096)
        ctx.decode(toks[:16], 0)                                           # buffers
        best = 1e9
        for _ in range(2):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(0, n, 512):
                ctx.decode(toks[i:i + 512], i)
            best = min(best, time.perf_counter() - t0)
        ctx.close()
        E, F, L, Ekv = CFG_8B["E"], CFG_8B["F"], CFG_8B["L"], CFG_8B["Hkv"] * (CFG_8B["E"] // CFG_8B["H"])
        flop_tok = 2.0 * L * (E * (E + 2 * Ekv) + E * E + 3 * E * F)       # the layers' mat-muls (lm_head runs for the last token only)
        tfl = flop_tok * n / best / 1e12
        sec["config3"] = dict(workload="Llama-3-8B Q4_K_M shapes, 2048-token prompt, micro-batches of 512, n_ctx 4096 (exact-integer MFMA prefill)", value=round(n / best, 1), unit="tokens/s",
                              tflops=round(tfl, 1), mfma_peak_tflops=2500.0, mfma_peak_frac=round(tfl / 2500.0, 4), ms=round(best * 1e3, 2))
    except Exception as e:
        sec["config3"] = dict(skipped="failed: %r" % (e,))
    try:                                                                   # ---- config 5
        sec["config5"] = bridge_longctx_rate()
    except Exception as e:
        sec["config5"] = dict(skipped="failed: %r" % (e,))
    try:                                                                   # ---- config 4, N = 1
        import shutil
        p70 = model_path("70b")
        free = shutil.disk_usage(os.path.dirname(p70)).free
        if not os.path.exists(p70 + ".done") and free < (48 << 30):
            sec["config4_n1"] = dict(skipped="no room for the 42 GB synthetic GGUF (%s has %.0f GB free)" % (os.path.dirname(p70), free / 2 ** 30))
        elif time.time() - t_all > 120:
            sec["config4_n1"] = dict(skipped="time budget of the secondary legs used up")
        else:
            ensure_model(p70, 0, "70b")
            m = booster_amd.Model(p70, device=0); ctx = booster_amd.Context(m, 512)
            prompt = [(7919 * i + 13) % CFG_70B["V"] for i in range(N_PROMPT)]
            ctx.decode(prompt[:8], 0); ctx.decode(prompt, 0)
            ctx.generate_greedy(N_PROMPT, 4)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            ctx.generate_greedy(N_PROMPT + 4, 32)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            l, _, _ = ctx.profile_step_kinds(N_PROMPT + 36)
            kvb = 2 * CFG_70B["L"] * CFG_70B["Hkv"] * 128 * 2
            bpt = m.weight_bytes + kvb * (N_PROMPT + 20)
            sec["config4_n1"] = dict(workload="the whole Llama-3-70B Q4_K_M (80 layers, %.1f GB of weights) on one MI355X, greedy decode, 128-token prompt" % (m.weight_bytes / 1e9),
                                     value=round(32 / dt, 2), unit="tokens/s", ms_per_token=round(dt / 32 * 1e3, 3), bytes_per_token=int(bpt),
                                     frac_of_hbm_roofline_tokens=round(32 / dt * bpt / (HBM_PEAK_GBS * 1e9), 4), launches_per_token=int(sum(l[:7])))
            ctx.close(); m.close()
            try:
                os.remove(p70); os.remove(p70 + ".done")                  # 42 GB of tmpfs: do not leave it behind for whatever runs next on the box
            except OSError:
                pass
    except Exception as e:
        sec["config4_n1"] = dict(skipped="failed: %r" % (e,))
    sec["seconds"] = round(time.time() - t_all, 1)
    return sec


def bridge_longctx_rate(n_pos=7900):
    """BASELINE config 5 as specified: Mistral-7B shape, all Q6_K, 8 K context, Janus sampling — through include/booster_bridge.h's nine symbols (ctypes
    stands where cgo would).  The decode rate at ~n_pos cached positions is the difference of two requests on the same prompt (n_predict 24 and 152): the
    prompt evaluation, tokenisation and sampler set-up cancel.  Round 5: both pods are warmed first, the pair is repeated three times (median, min / max), and
    the level-1 greedy rate at the same cached length is reported beside it (the first version timed pod 2's first-request allocations)."""
    import ctypes as C
    from booster_amd import gguf, build
    path = os.path.join(os.path.dirname(model_path("m7q6k")), "bamd_bench_m7q6k_vocab.gguf")
    if not os.path.exists(path + ".done"):
        v = gguf.synthetic_bpe_vocab(n_merges=2000)
        ctrl = v["tokens"][-4:]; toks = v["tokens"][:-4]; types = v["types"][:-4]
        while len(toks) < 32000 - 4:
            toks.append("\u0120fill%d" % len(toks)); types.append(1)
        v["tokens"] = toks + ctrl; v["types"] = types + [3] * 4
        n = len(v["tokens"]); v["bos_token_id"] = n - 4; v["eos_token_id"] = n - 3
        gguf.write_synthetic_llama(path, E=4096, H=32, Hkv=8, L=32, F=14336, V=n, theta=10000.0, seed=7, reuse_layers=True, vocab=v,
                                   type_fn=lambda name, il: gguf.Q6_K, embd_type=gguf.Q6_K)
        open(path + ".done", "w").write("ok")
    L = C.CDLL(build.build())
    i, f, u = C.c_int, C.c_float, C.c_uint32
    L.initContext.restype = C.c_void_p
    L.initContext.argtypes = [i, C.c_char_p, i, i, i, i, i, i, i, i, C.c_int32, f, f, f, i, f, f, f, i, C.c_int32, C.c_int32, f, f, f, u, C.c_char_p]
    L.doInference.restype = C.c_int64; L.doInference.argtypes = [i, C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]
    L.getPromptTokenCount.restype = C.c_int64; L.getPromptTokenCount.argtypes = [C.c_char_p]
    L.init(b"", b"")
    unit = "the quick brown fox jumps over the lazy dog and then "
    # Two pods (n_predict is a context parameter: cpp/bridge.cpp:723-786), both on this GPU.  Each gets ONE discarded warm-up request with the very prompt
    # (its first doInference allocates the prefill buffers and the attention scratch; the KV cache is cleared per request by contract, bridge.cpp:459), then
    # three timed requests, the pods alternating; the decode rate is the MEDIAN of the three differences (long request - short request), min / max beside it.
    ctxs = {}
    for idx, n_predict in ((1, 24), (2, 152)):
        c = L.initContext(idx, path.encode(), 4, 512, 100, 0, 0, 0, 8192, n_predict, 0, 0.0, 0.0, 0.8, 40, 0.9, 1.0, 1.1, 64, 1, 200, 0.97, 0.99, 0.96, 42, b"")
        if not c:
            raise RuntimeError("initContext failed")
        ctxs[n_predict] = (idx, c)
    L.doInference(1, ctxs[24][1], b"probe", b"s", (unit * 8).encode())     # size the prompt: tokens per repetition of the unit, from a short request's count
    per = max(L.getPromptTokenCount(b"probe") / 8.0, 1.0)
    prompt = (unit * int(n_pos / per)).encode()

    def request(n_predict, tag):
        idx, c = ctxs[n_predict]
        job = b"cfg5_%d_%s" % (n_predict, tag)
        t0 = time.perf_counter()
        n = L.doInference(idx, c, job, b"s", prompt)
        return time.perf_counter() - t0, int(n), int(L.getPromptTokenCount(job))

    for n_predict in (24, 152):
        request(n_predict, b"warm")
    pairs = []
    for r in range(3):
        ta, na, pa = request(24, b"r%d" % r)
        tb, nb, pb = request(152, b"r%d" % r)
        gen = (nb - pb) - (na - pa)
        if gen <= 0:
            raise RuntimeError("the two requests generated %d and %d tokens (an end-of-generation token cut one short)" % (na - pa, nb - pb))
        pairs.append(dict(ms=(tb - ta) / gen * 1e3, ta=ta, tb=tb, gen=[na - pa, nb - pb], prompt=pb, total=nb))
    ms_all = sorted(p_["ms"] for p_ in pairs)
    ms = ms_all[1]
    pb, nb_tot = pairs[0]["prompt"], pairs[0]["total"]
    E, F, Lr, V = 4096, 14336, 32, 32000
    W = (Lr * (E * (E + 2 * 1024) + E * E + 3 * E * F) + V * E) // 256 * 210
    bpt = W + 2 * Lr * 1024 * 2 * (pb + (nb_tot - pb) // 2)
    out = dict(workload="Mistral-7B shape, every matrix Q6_K, n_ctx 8192, through the nine bridge symbols with Janus sampling (device prefilter): decode at %d cached positions" % pb,
               value=round(1e3 / ms, 2), unit="tokens/s", ms_per_token=round(ms, 3), prompt_tokens=pb, generated=pairs[0]["gen"], bytes_per_token=int(bpt),
               frac_of_hbm_roofline_tokens=round(1e3 / ms * bpt / (HBM_PEAK_GBS * 1e9), 4),
               repeats=dict(n=3, tokens_per_s=dict(min=round(1e3 / ms_all[2], 2), median=round(1e3 / ms_all[1], 2), max=round(1e3 / ms_all[0], 2)),
                            request_seconds=[[round(p_["ta"], 3), round(p_["tb"], 3)] for p_ in pairs],
                            note="both pods warmed by one discarded request of the same prompt; value = median of three (152-token request - 24-token request) differences (128 tokens: round 6 — with 64 a 3 ms wobble of the 0.8 s prompt evaluation moved the rate by 2 %)"))
    # level-1 cross-check on the same GGUF at the same cached length: Context.generate_greedy (device-side greedy loop, no bridge, no Janus) — the difference
    # to `value` is what the bridge's per-token host work (sampler, detokenisation, status text) costs
    try:
        import booster_amd
        import torch
        m = booster_amd.Model(path, device=0)
        ctx = booster_amd.Context(m, 8192)
        toks = [(7919 * i + 13) % m.n_vocab for i in range(pb)]
        for i in range(0, pb, 512):
            ctx.decode(toks[i:i + 512], i)
        ctx.generate_greedy(pb, 8)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        ctx.generate_greedy(pb + 8, 64)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        out["level1_greedy"] = dict(value=round(64 / dt, 2), unit="tokens/s", ms_per_token=round(dt / 64 * 1e3, 3), cached_positions=pb + 8,
                                    note="Context.generate_greedy (include/bamd.h) at the same cached length: the bridge + Janus overhead is the difference to `value`")
        ctx.close(); m.close()
    except Exception as e:
        out["level1_greedy"] = dict(skipped="failed: %r" % (e,))
    return out


def emit(rank, dist, result, model_name, N, steps, warmup):
    """rank 0 prints the ONE JSON line, after every rank has left the process group"""
    out = None
    if rank == 0:
        out = dict(metric="decode tokens/sec " + model_name, value=result.pop("value"), unit="tokens/s", n_gpus=N, steps=steps,
                   warmup=warmup, ms_per_step=result.pop("ms_per_step"), higher_is_better=True, scaling=result.pop("scaling"),
                   vs_baseline=None, dtype="int8xint4/6 dot -> f32 (Q4_K/Q6_K weights x Q8_K activations), f16 KV", data="synthetic")
        out.update(result)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    # The JSON line must be the LAST thing on stdout: RCCL writes a version banner through C stdio, which would otherwise be flushed
    # at process exit, after Python's own buffer.  Drain C stdio first, then print and flush as the last act of the program (a normal
    # return, so that a profiler attached to the process still writes its output at exit).
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stderr.flush()
    if rank == 0:
        sys.stdout.write(json.dumps(out) + "\n")
    sys.stdout.flush()


def self_launch(N, argv):
    """re-exec this script under torch.distributed.run with N ranks on 127.0.0.1 (a free port); the ranks' stdout is ours: rank 0's JSON line"""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(N), "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd)


if __name__ == "__main__":
    main()
