"""The GPU cases of tests/test_gpu_f64_guard.py that run on a vector WITH TEETH (tests/golden/f64_teeth_kats.npz, gen_f64_teeth_kats.py): inputs, the op call
and BOTH expectations of every case — with the sequential mean (what the reference computes and the kernel's fallback must give) and with the mean of the
site's own tree (what a kernel gives that skipped the fallback or summed it in the tree's order).  tests/test_f64_teeth.py asserts on the CPU that the two
differ in at least one output element of every case; tests/test_gpu_f64_guard.py runs the op and compares with the first, bit for bit.

The arithmetic of the expectations is the oracle's rms_norm (sequential mean), normed_with_mean (tree mean; held to the oracle bit for bit where it is given
the sequential mean) and the restatements tests/float_ref.py, legacy_ref.py, legacy1_ref.py, iq4nl_ref.py and the oracle's mul_mat_q: never the code under test.

A case is a function (po, rng, K) -> dict(expect = activation vector -> output, run = (bamd, x or X, w, eps) -> output, and what names its kernel:
trace = (segments [(type, rows)], epilogue, mode, mangled-name part) for bamd_trace_mv, mfma = the weight type whose matrix-core launch counter must move,
switch = the setter that routes the prompt mat-mul there).  batch: the op takes T = 3 token rows and only token 1 is the constructed vector."""
import contextlib
import os
import sys
import types

import numpy as np

import float_ref as fr
import iq4nl_ref as nl
import legacy1_ref as l1
import legacy_ref as lg
from booster_amd.gguf import random_float_tensor, random_iq4_nl_tensor, random_kquant_tensor, random_q0_tensor, random_q1_tensor
from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import f64_order_search as fs  # noqa: E402

F32, F16, BF16, NL, Q8_0, Q4_0, Q4_1, Q4_K = fr.F32, fr.F16, fr.BF16, nl.IQ4_NL, lg.Q8_0, lg.Q4_0, l1.Q4_1, 12
TNAME = {F32: "f32", F16: "f16", BF16: "bf16", NL: "iq4_nl", Q8_0: "q8_0", Q4_0: "q4_0", Q4_1: "q4_1", Q4_K: "q4_k"}
PRO_NORM, EPI_STORE, EPI_SILU_MUL, EPI_ARGMAX = 1, 0, 2, 3
NT = 8
CASES = {}                                                    # id -> (site, K, batch, builder), in the order of the issue's sections


def load():
    return np.load(os.path.join(GOLDEN, "f64_teeth_kats.npz"))


def teeth_vector(tk, site, K):
    """the vector of a (site, length) with the CPU-side proof of its four conditions (gen_f64_teeth_kats.py): the guard fires on it whatever the tree, and the
    site's tree rounds to another f32 mean and another f32 scale.  -> x, eps, sequential mean, tree mean"""
    name = "%s_%d" % (site, K)
    x, eps = tk["x_" + name], float(tk["eps"])
    t = fs.terms(x)
    o = fs.sum_orders(t)
    tree = fs.SITE_TREES[site](t)
    m_seq, m_tree = np.float32(fs.mean64(o["seq"], K)), np.float32(fs.mean64(tree, K))
    assert x.size == K and int(fs.dist_units(fs.mean64(o["seq"], K))) <= fs.NEAR_UNITS, name
    assert all(fs.guard_fires(s, K) for s in list(o.values()) + [tree]), name
    assert m_seq.view(np.uint32) == tk["mean_seq_" + name].view(np.uint32) != m_tree.view(np.uint32) == tk["mean_tree_" + name].view(np.uint32), name
    assert fs.scale32(m_seq, eps).view(np.uint32) != fs.scale32(m_tree, eps).view(np.uint32), name
    return x, eps, m_seq, m_tree


def quiet_vector(rng, K):
    """a random vector on which NO tree fires: the sequential mean is further from a boundary than the band 2 K + 8 plus the reordering error 2 K"""
    while True:
        x = (rng.standard_normal(K) * 2).astype(np.float32)
        if int(fs.dist_units(fs.mean64(fs.sum_seq(fs.terms(x)), K))) > 4 * K + 8:
            return x


def normed_with_mean(x, w, mean32, eps):
    """(x * scale) * w with scale = 1 / sqrtf(mean + eps) in f32: ggml_vec_scale_f32 then ggml_mul (llama.cpp:7940-7950), for a GIVEN f32 mean"""
    x = np.asarray(x, np.float32)
    return ((x * fs.scale32(mean32, eps)).astype(np.float32) * np.asarray(w, np.float32)).astype(np.float32)


MAX_WEIGHT_DRAWS = 20000


def act_form(po, t):
    """what the kernels of weight type t make of the normed vector before any weight meets it: the f32 vector itself (F32 / F16), its bf16 bits (BF16), Q8_0 /
    Q8_1 / Q8_K blocks.  The forms that round hide most one-ulp changes of the vector: of a bf16 value about one in 2^16, of a Q8_0 block's f16 scale about
    one in 2^13 — at K = 256 a vector in two hundred would show the other scale in its bf16 bits, far beyond the 64 seeds of a pair.  The norm weights
    are an input of the case that does not enter the sum: built() draws them (fixed seed) until the form of the two normed vectors differs"""
    if t == BF16:
        return fr.bf16_bits
    if t in (F32, F16):
        return lambda a: a.view(np.uint32)
    if t in (Q4_1, l1.Q5_1):
        return l1.quantize_row_q8_1
    if t in (NL, Q8_0, Q4_0, lg.Q5_0):
        return lg.quantize_row_q8_0
    return po.quantize_q8_K


def norm_weights(rng, K):
    return (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)           # random: the weights do not enter the sum


def case(cid, site, K, batch=False):
    def deco(f):
        assert cid not in CASES
        CASES[cid] = (site, K, batch, f)
        return f
    return deco


_BUILT = {}


def built(po, tk, cid):
    """the case with its inputs and both expectations, once per process"""
    if cid not in _BUILT:
        site, K, batch, f = CASES[cid]
        x1, eps, m_seq, m_tree = teeth_vector(tk, site, K)
        rng = np.random.default_rng([20261020] + list(cid.encode()))
        c = types.SimpleNamespace(**dict(dict(id=cid, site=site, K=K, batch=batch, eps=eps, trace=None, mfma=None, switch=None, argmax=False), **f(po, rng, K)))
        form = act_form(po, c.form)
        for _ in range(MAX_WEIGHT_DRAWS):
            c.w = norm_weights(rng, K)
            a_seq = (po.rms_norm(x1, eps) * c.w).astype(np.float32)
            a_tree = normed_with_mean(x1, c.w, m_tree, eps)
            if not np.array_equal(form(a_seq), form(a_tree)):
                break
        else:
            raise AssertionError("%s: no norm weights under which the activation form shows the other scale" % cid)
        assert np.array_equal(a_seq.view(np.uint32), normed_with_mean(x1, c.w, m_seq, eps).view(np.uint32)), "normed_with_mean is not the oracle's RMSNorm"
        if batch:
            c.x = np.stack([quiet_vector(rng, K), x1, quiet_vector(rng, K)])
            quiet = [(po.rms_norm(c.x[i], eps) * c.w).astype(np.float32) for i in (0, 2)]
            c.want_seq = np.stack([c.expect(a) for a in (quiet[0], a_seq, quiet[1])])
            c.want_tree = c.want_seq.copy()
            c.want_tree[1] = c.expect(a_tree)
        else:
            c.x = x1
            c.want_seq, c.want_tree = c.expect(a_seq), c.expect(a_tree)
        for a in (c.x, c.w, c.want_seq, c.want_tree):
            a.setflags(write=False)
        _BUILT[cid] = c
    return _BUILT[cid]


@contextlib.contextmanager
def switched(bamd, name):
    """a prompt mat-mul switch on for the block, then back to what the library read from the environment when it was loaded"""
    setter = getattr(bamd, "set_prefill_" + name)
    setter(True)
    try:
        yield
    finally:
        setter(os.environ.get("BAMD_PREFILL_" + name.upper(), "")[:1] == "1")


def ref_mul_mat(po, t, W, rows, K, a):
    if t in fr.TYPES:
        return fr.mul_mat(t, W, rows, K, a)
    if t == NL:
        return nl.mul_mat(W, rows, K, a)
    if t in (Q8_0, Q4_0, lg.Q5_0):
        return lg.mul_mat(t, W, rows, K, a)
    if t in (Q4_1, l1.Q5_1):
        return l1.mul_mat(t, W, rows, K, a)
    return po.mul_mat_q(t, W, rows, K, a, nthreads=NT)[0]


def rand_w(t, K, rows, rng):
    if t in fr.TYPES:
        return random_float_tensor(t, K, rows, rng, amp=4.0)
    if t == NL:
        return random_iq4_nl_tensor(K, rows, rng)
    if t in (Q8_0, Q4_0):
        return random_q0_tensor(t, K, rows, rng)
    if t == Q4_1:
        return random_q1_tensor(t, K, rows, rng)
    return random_kquant_tensor(t, K, rows, rng, amp=4.0)


def mv_kernel(t, epi, mode=0):
    """the part of the mangled kernel name a launch of type t must carry: <family kernel><.., PRO_NORM, epilogue>"""
    if t in fr.TYPES:
        return "matvec_flt_kernelILb%dELi%dELi%dE" % (t == BF16, PRO_NORM, epi)
    if mode == 2:
        return "matvec_q0_split_kernelILi%dELi%dE" % (PRO_NORM, epi)
    return "%sILb%dELi%dELi%dE" % ("matvec_b32_nl_kernel" if t == NL else "matvec_b32_kernel", t == Q4_1, PRO_NORM, epi)


# ---- the case families ------------------------------------------------------------------------------------------------------------------------
def mat_vec(t, rows, mode=0):
    """op_mul_mat_vec with the RMSNorm prologue.  rows 24: three row-groups; 13: two, the second ragged — workgroups of one busy wave and seven idle ones"""
    def f(po, rng, K):
        W = rand_w(t, K, rows, rng)
        pad = (rows + 7) // 8 * 8
        return dict(form=t, expect=lambda a: ref_mul_mat(po, t, W, rows, K, a), trace=([(t, pad)], EPI_STORE, mode, mv_kernel(t, EPI_STORE, mode)),
                    run=lambda bamd, x, w, eps: bamd.op_mul_mat_vec(t, W, rows, K, x, norm_w=w, eps=eps, mode=mode))
    return f


def gate_up(t, rows):
    def f(po, rng, K):
        Wg, Wu = rand_w(t, K, rows, rng), rand_w(t, K, rows, rng)
        return dict(form=t, expect=lambda a: (po.silu(ref_mul_mat(po, t, Wg, rows, K, a)) * ref_mul_mat(po, t, Wu, rows, K, a)).astype(np.float32),
                    trace=([(t, rows), (t, rows)], EPI_SILU_MUL, 0, mv_kernel(t, EPI_SILU_MUL)),
                    run=lambda bamd, x, w, eps: bamd.op_ffn_gate_up(t, Wg, Wu, rows, K, x, norm_w=w, eps=eps))
    return f


def lm_head(t, rows):
    """the arg-max epilogue: run gives (logits, row); the runner checks the row and its key against the expectation"""
    def f(po, rng, K):
        W = rand_w(t, K, rows, rng)
        return dict(form=t, expect=lambda a: ref_mul_mat(po, t, W, rows, K, a), argmax=True, trace=([(t, rows)], EPI_ARGMAX, 0, mv_kernel(t, EPI_ARGMAX)),
                    run=lambda bamd, x, w, eps: bamd.op_mul_mat_vec_argmax(t, W, rows, K, x, norm_w=w, eps=eps))
    return f


def fused(layout, mode=0):
    """op_fused_qkv over the segments [(type, rows)].  With 8 rows in the first segment and 16 behind it the launch has three row-groups = three workgroups,
    of which two have nothing in segment 0: their prologue runs in front of a later segment (pro_done), the idle waves' behind the last"""
    def f(po, rng, K):
        segs = [(t, rand_w(t, K, r, rng), r) for t, r in layout]
        kernel = mv_kernel(NL if any(t == NL for t, _ in layout) else layout[0][0], EPI_STORE, mode)
        return dict(form=layout[0][0], expect=lambda a: np.concatenate([ref_mul_mat(po, t, W, r, K, a) for t, W, r in segs]), trace=(list(layout), EPI_STORE, mode, kernel),
                    run=lambda bamd, x, w, eps: bamd.op_fused_qkv(segs, K, x, w, eps=eps, mode=mode))
    return f


def prompt(t, rows, impl, switch=None):
    """op_mul_mat_batch at T = 3 (a workgroup of the activation kernel per token: one takes the fallback between two that do not).  impl 2 reads the f16 record
    of the quantiser (blob16) or, F32 / F16, the f32 form on the matrix cores"""
    def f(po, rng, K):
        W = rand_w(t, K, rows, rng)
        return dict(form=t, expect=lambda a: ref_mul_mat(po, t, W, rows, K, a), switch=switch, mfma=t if impl == 2 and switch else None,
                    run=lambda bamd, X, w, eps: bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=eps, impl=impl))
    return f


def quantiser(q1):
    def f(po, rng, K):
        return dict(form=Q4_1 if q1 else Q8_0, expect=l1.quantize_row_q8_1 if q1 else lg.quantize_row_q8_0,
                    run=lambda bamd, x, w, eps: (bamd.op_quantize_q8_1 if q1 else bamd.op_quantize_q8_0)(x, norm_w=w, eps=eps))
    return f


# B: flt_act (bamd_flt_device.h), inlined into matvec_flt_kernel, act_bf16_test_kernel and act_batch_flt_kernel
for _K in (256, 768, 4096):
    case("act_bf16-K%d" % _K, "flt", _K)(lambda po, rng, K: dict(form=BF16, expect=fr.bf16_bits, run=lambda bamd, x, w, eps: bamd.op_act_bf16(x, norm_w=w, eps=eps)))
for _t in (F32, F16, BF16):
    case("mat_vec-%s-K4096" % TNAME[_t], "flt", 4096)(mat_vec(_t, 24))
case("mat_vec-f16-K3072", "flt", 3072)(mat_vec(F16, 24))                                 # K no power of two: the mean is a division
for _t in (F16, BF16):
    case("gate_up-%s-K768" % TNAME[_t], "flt", 768)(gate_up(_t, 24))
for _t in (F16, BF16):
    case("lm_head-%s-K4096" % TNAME[_t], "flt", 4096)(lm_head(_t, 24))
case("fused-f32_f16-K3072", "flt", 3072)(fused(((F32, 8), (F16, 16))))
for _t in (F32, F16, BF16):
    case("prompt-%s-impl0" % TNAME[_t], "flt", 4096, batch=True)(prompt(_t, 24, 0))
for _t in (F32, F16):
    case("prompt-%s-impl2" % TNAME[_t], "flt", 4096, batch=True)(prompt(_t, 24, 2, "flt"))

# C: the instantiations of ActProQ0::finish_q0 (bamd_b32_device.h) that had no firing vector
case("mat_vec-iq4_nl-mode1", "q0", 4096)(mat_vec(NL, 13, 1))
case("fused-iq4_nl_q8_0-mode1", "q0", 4096)(fused(((NL, 8), (Q8_0, 16)), 1))
case("prompt-iq4_nl-impl0", "q0", 4096, batch=True)(prompt(NL, 13, 0))
case("prompt-iq4_nl-impl2", "q0", 4096, batch=True)(prompt(NL, 13, 2, "nl"))
for _t in (Q8_0, Q4_1, NL):
    case("gate_up-%s-K768" % TNAME[_t], "q0", 768)(gate_up(_t, 16))
for _t in (Q8_0, Q4_1, NL):
    case("lm_head-%s-K4096" % TNAME[_t], "q0", 4096)(lm_head(_t, 24))
case("prompt-q8_0-impl2", "q0", 4096, batch=True)(prompt(Q8_0, 13, 2, "q0"))            # the blob16 branch of quantize_batch_b32_kernel
case("prompt-q4_1-impl2", "q0", 4096, batch=True)(prompt(Q4_1, 13, 2, "q1"))
for _m in (1, 2):                                                                      # mode 2: matvec_q0_split_kernel, whole workgroups skip segment 0
    case("fused-q8_0_q4_0-K8192-mode%d" % _m, "q0", 8192)(fused(((Q8_0, 8), (Q4_0, 16)), _m))

# D: the cases of test_quantize_batch, test_q8_0_family and test_q8_1_family again, on a vector of their site on which a wrong sum shows
for _i in (0, 2):
    case("quantize_batch-q4_k-impl%d" % _i, "actpro", 4096, batch=True)(prompt(Q4_K, 64, _i))
FAMILY = {}
for _n, _t, _q1, _modes in (("q8_0", Q8_0, False, (1, 2)), ("q8_1", Q4_1, True, (1,))):
    FAMILY[_n] = ["family-%s-quantiser" % _n] + ["family-%s-mat_vec-mode%d" % (_n, m) for m in _modes] + ["family-%s-prompt-impl0" % _n]
    case(FAMILY[_n][0], "q0", 4096)(quantiser(_q1))
    for _m in _modes:
        case("family-%s-mat_vec-mode%d" % (_n, _m), "q0", 4096)(mat_vec(_t, 13, _m))
    case(FAMILY[_n][-1], "q0", 4096, batch=True)(prompt(_t, 13, 0))
FAMILY_IDS = {c for ids in FAMILY.values() for c in ids}
