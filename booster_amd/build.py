"""Builds booster_amd/lib/libbooster_amd.so for gfx950 with hipcc (in-tree, so the .so travels with the repo).

    python -m booster_amd.build [--force]
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "lib", "libbooster_amd.so")
# the kernels of a decode step are ALSO built as raw gfx950 code objects (same sources, same flags) and embedded in the library: bamd_aql.cpp loads them through
# HSA and replays a step from the library's own AQL queue (csrc/bamd_aql.h)
DECODE_KERNEL_SOURCES = ["bamd_matvec.hip", "bamd_matvec_b32_q0.hip", "bamd_matvec_b32_q1.hip", "bamd_matvec_b32_nl.hip", "bamd_matvec_flt.hip", "bamd_matvec_fast_a.hip", "bamd_matvec_fast_b.hip", "bamd_attention.hip", "bamd_colaunch.hip"]
SOURCES = ["bamd_aql.cpp", "bamd_matvec.hip", "bamd_matvec_b32_q0.hip", "bamd_matvec_b32_q1.hip", "bamd_matvec_b32_nl.hip", "bamd_matvec_flt.hip", "bamd_matvec_fast_a.hip", "bamd_matvec_fast_b.hip", "bamd_attention.hip", "bamd_attention_mfma.hip", "bamd_attention_gs.hip", "bamd_colaunch.hip", "bamd_prefill.hip", "bamd_prefill_b32.hip", "bamd_prefill_b32_nl.hip", "bamd_prefill_flt.hip", "bamd_prefill2.hip", "bamd_prefill2_b32.hip", "bamd_prefill2_flt.hip", "bamd_prefill2_bf16.hip", "bamd_prefill_family.cpp", "bamd_sampler.hip", "bamd_engine.cpp", "bamd_ops.cpp", "bamd_gguf.cpp", "bamd_vocab.cpp", "bamd_bridge.cpp"]
HEADERS = ["bamd_aql.h", "bamd_engine_internal.h", "bamd_formats.h", "bamd_kernels.h", "bamd_device.h", "bamd_b32_device.h", "bamd_prefill_b32.h", "bamd_prefill_valu.h", "bamd_prefill_family.h", "bamd_flt_device.h", "bamd_bf16_range.h", "bamd_matvec_b32.h", "bamd_matvec_core.h", "bamd_mv_select.h", "bamd_attn_fused.h", "bamd_attn_batch.h", "bamd_mfma_common.h", "bamd_gguf.h", "bamd_vocab.h", "bamd_unicode_tables.h", "../../include/bamd.h", "../../include/booster_bridge.h"]
# -ffp-contract=off: the numerics contract (bit-parity with the reference CPU path) forbids implicit FMA fusion.
# -fno-slp-vectorize (decode kernels only, NO_SLP): SLP packs neighbouring f32 multiplies into v_pk_mul_f32, whose operands need
# even-aligned register pairs: the copies it adds sit right behind the loads (a full s_waitcnt before the weight ring could be
# requested) and packed f32 is no faster there.  The prefill kernels keep SLP: their f32 chains run on float4 accumulators, where
# v_pk_fma_f32 halves the instruction count (same IEEE fma per element).
NO_SLP = ("bamd_matvec.hip", "bamd_matvec_b32_q0.hip", "bamd_matvec_b32_q1.hip", "bamd_matvec_b32_nl.hip", "bamd_matvec_flt.hip", "bamd_matvec_fast_a.hip", "bamd_matvec_fast_b.hip", "bamd_attention.hip", "bamd_colaunch.hip", "bamd_attention_gs.hip", "bamd_prefill2_bf16.hip")
# gfx950 kernarg preload for the decode mat-vec kernels: their leading scalar parameters (BAMD_LEAD_PARAMS: activation / weight pointers, K, eps)
# arrive in SGPRs at wave launch, so the first requests do not wait for an s_load of the argument block (+0.3 % decode, measured)
KERNARG_PRELOAD = {"bamd_matvec_fast_a.hip": ["-mllvm", "-amdgpu-kernarg-preload-count=16"], "bamd_matvec_fast_b.hip": ["-mllvm", "-amdgpu-kernarg-preload-count=16"]}
# the Q8_0 / Q4_0 / Q5_0, the Q4_1 / Q5_1 and the IQ4_NL instances of the prompt kernel chain every MFMA result on the VALU: results in VGPRs (the default puts them in AGPRs and copies each one out)
MFMA_VGPR_FORM = {"bamd_prefill2_b32.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]}
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-fvisibility=hidden", "-Wno-unused-result", "-Wno-unused-value"]


LIB_TIMING = os.path.join(HERE, "lib", "libbooster_amd_timing.so")      # -DBAMD_TIMING: kernels write phase stamps (tools/timeline.py)


def flags_of(s, timing=False, extra=()):
    """the compile flags of source file s (also what tools/codeobj_diff.py compiles with)"""
    return FLAGS + (["-fno-slp-vectorize"] if s in NO_SLP else []) + KERNARG_PRELOAD.get(s, []) + MFMA_VGPR_FORM.get(s, []) + (["-DBAMD_TIMING"] if timing else []) + list(extra)


def _stale(lib=LIB):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False, timing=False, variant=None, extra=()):
    """variant / extra: experiment builds — lib/libbooster_amd_<variant>.so compiled with the extra flags (select with BAMD_LIB)"""
    lib = LIB_TIMING if timing else LIB
    if variant:
        lib = os.path.join(HERE, "lib", "libbooster_amd_%s.so" % variant)
    if not force and not _stale(lib):
        return lib
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(HERE, "lib", variant) if variant else os.path.join(HERE, "lib", "timing") if timing else os.path.join(HERE, "lib")
    os.makedirs(objdir, exist_ok=True)
    objs = []
    procs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        if not os.path.exists(src):
            continue
        obj = os.path.join(objdir, os.path.splitext(s)[0] + ".o")
        objs.append(obj)
        cmd = [hipcc] + flags_of(s, timing, extra) + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd)))
    hsacos = []
    for s in DECODE_KERNEL_SOURCES:
        co = os.path.join(objdir, os.path.splitext(s)[0] + ".hsaco")
        hsacos.append((os.path.splitext(s)[0], co))
        cmd = [hipcc] + [f for f in flags_of(s, timing, extra) if f != "-fPIC"] + ["--genco", "--no-gpu-bundle-output", os.path.join(CSRC, s), "-o", co]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd, stderr=subprocess.DEVNULL if not verbose else None)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise RuntimeError("compile failed: " + " ".join(cmd))
    # the code objects as read-only data of the library + the table bamd_aql.cpp walks
    blob = os.path.join(objdir, "bamd_hsaco_blob.cpp")
    with open(blob, "w") as f:
        f.write("// generated by booster_amd/build.py: the decode kernels' gfx950 code objects, embedded\n")
        f.write('__asm__(".section .rodata\\n"\n')
        for i, (name, co) in enumerate(hsacos):
            f.write('        ".p2align 12\\nbamd_hsaco_%d_begin:\\n.incbin \\"%s\\"\\nbamd_hsaco_%d_end:\\n"\n' % (i, co, i))
        f.write('        ".text\\n");\n')
        f.write("struct bamd_hsaco_entry { const unsigned char * begin, * end; const char * name; };\n")
        f.write('extern "C" {\n')
        for i in range(len(hsacos)):
            f.write("extern const unsigned char bamd_hsaco_%d_begin[], bamd_hsaco_%d_end[];\n" % (i, i))
        f.write("extern const bamd_hsaco_entry bamd_hsaco_table[] = {\n")
        for i, (name, co) in enumerate(hsacos):
            f.write('    { bamd_hsaco_%d_begin, bamd_hsaco_%d_end, "%s" },\n' % (i, i, name))
        f.write("};\nextern const int bamd_hsaco_count = %d;\n}\n" % len(hsacos))
    blob_o = os.path.join(objdir, "bamd_hsaco_blob.o")
    cmd = ["/usr/bin/g++", "-c", "-fPIC", "-O1", "-fvisibility=hidden", blob, "-o", blob_o]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    objs.append(blob_o)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs + ["-L/opt/rocm/lib", "-lhsa-runtime64"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return lib


if __name__ == "__main__":
    _v = sys.argv[sys.argv.index("--variant") + 1] if "--variant" in sys.argv else None
    print(build(force="--force" in sys.argv, verbose="--verbose" in sys.argv, timing="--timing" in sys.argv, variant=_v, extra=[a for a in sys.argv[1:] if a.startswith("-D") or a.startswith("-f") or a.startswith("-m") or a.startswith("-amdgpu")]))
