"""GPU: the SEQUENTIAL fallback of every double-precision sum, per kernel.  f32_rounding_safe (bamd_device.h) sends a reduction down the reference's
order when the tree order could show in the f32 result — about 1e-5 of natural reductions, so seeded tests never take it.  The fallback is hand-written
at ten sites, each with its own barriers and its own storage of the exponentials.  Every case here feeds one site a CONSTRUCTED input
(tests/golden/f64_order_kats.npz, f64_teeth_kats.npz, f64_softmax_kats.npz; tools/f64_order_search.py, tools/f64_softmax_search.py) whose sequential value sits within 8 units
of an f32 rounding boundary: any tree of the same terms lies inside the guard's band, so the fallback runs whatever the kernel's tree is.  Each case
  - asserts on the CPU that the guard fires on its input (and, where the case says so, that the neighbouring rows do NOT fire: their sequential value is
    further from a boundary than the band plus the largest reordering error);
  - asserts which kernel the shape lands on (bamd_trace_matvec / bamd_trace_attn_wo with the device's CU count, or the impl / ld / mode argument);
  - compares every output with the oracle bit for bit: outputs, both KV caches, probabilities where the entry point returns them.  No tolerances.
A shape the launcher declines or routes elsewhere FAILS.  Mat-vec cases call the launch three times (the fallback adds barriers): all three must match.

  site                          cases
  ActPro::finish           bamd_device.h              test_fused_qkv_fast, test_generic_kernels, test_gate_up, test_lm_head_k8192, test_quantize_batch
  ActProQ0::finish_q0      bamd_b32_device.h          test_q8_0_family, test_q8_1_family, test_legacy_family_teeth; test_teeth: matvec_b32_nl_kernel and
                                                      matvec_b32_kernel with the STORE / SILU_MUL / ARGMAX epilogues, launches whose first segment has no row-group
                                                      for a workgroup (also matvec_q0_split_kernel), quantize_batch_b32_kernel's f32 and f16 (blob16) records
  flt_act                  bamd_flt_device.h          test_teeth: matvec_flt_kernel<BF, PRO_NORM, EPI> (STORE / SILU_MUL / ARGMAX x two activation forms, an F32 segment
                                                      beside an F16 one), act_bf16_test_kernel, act_batch_flt_kernel<true, BF> in front of the VALU and of the
                                                      matrix-core prompt kernel
  attn_softmax_kernel     bamd_attention.hip         test_softmax_kernel (cached 96 / 4128, uncached 8224), test_softmax_kernel_cells (holes)
  attn_spv_kernel<NH>      bamd_attention.hip         test_spv (NH 1, 2, 4)
  attn_batch_kernel<GQH>   bamd_attn_batch.h          test_batch_valu (attn_batch_body, rows in LDS)
  attn_fused_body          bamd_attn_fused.h          test_fused (single launch), test_colaunch (attention || wo, COLAUNCH = true)
  attn_batch_gs_kernel     bamd_attn_batch.h          test_batch_scratch_rows (the same attn_batch_body, rows in the scratch block)
  attn_batch_mfma_kernel<GQ, false>                   test_batch_mfma, padded length <= 512: rows in LDS (64 and 448 positions)
  attn_batch_mfma_kernel<GQ, true>                    test_batch_mfma, padded length > 512: rows in the scratch block (576 positions; 64 and 576 under ld 18496)

Which RMSNorm cases can see a wrong VALUE (and not only a hang or a fault of the fallback): those whose vector rounds to another f32 mean and scale under the
site's own tree.  Of f64_order_kats.npz that holds for K3072 and K4096 (both trees of tools/f64_order_search.py SITE_TREES); at K8192 the mean differs and the scale
does not; at K256, K768 and K4096b no restated order differs.  The vectors of f64_teeth_kats.npz are chosen for it per (site, length), and tests/test_f64_teeth.py
shows on the CPU that the expected output of every case on them is another one under the tree's mean: test_teeth, test_quantize_batch_teeth, test_legacy_family_teeth.

Which attention kernel a shape lands on: the batched launches ask bamd_attention_batch_plan, whose scratch bytes are non-zero exactly when the rows live
in the scratch block (matrix cores: ld > 512 = LONG; VALU: ld > 18432 = attn_batch_gs_kernel), and the case fails where that differs from what it names.
The single-token paths have no such call: there the ratio and the long_path / want_probs argument decide (bamd_launch_attention: the default path is
attn_fused_kernel; the three-launch path runs attn_spv_kernel<NH> for gq 1 / 2 / 4 / 8 while its rows fit the LDS, attn_softmax_kernel for every other
ratio and for cell positions), which the cases state and cannot assert.

Softmax rows reach a kernel as dot products: q = c e_0 for the heads of one KV head (c = 1: the constructed row; c = 1/2: a quiet one), K rows = score x e_0
(f16-exact), identity RoPE.  Positions behind the constructed token hold further random scores, so every token of a micro-batch has a row of its own."""
import contextlib
import os
import sys

import numpy as np
import pytest

import booster_amd
import f64_teeth_cases as tc
import legacy1_ref as l1
import legacy_ref as lg
from bitcheck import assert_bits
from booster_amd.gguf import random_kquant_tensor, random_q0_tensor, random_q1_tensor
from conftest import GOLDEN, ROOT
from test_gpu_colaunch import device_cus, tag_of

sys.path.insert(0, os.path.join(ROOT, "tools"))
import f64_order_search as fs  # noqa: E402
import f64_softmax_search as ss  # noqa: E402

pytestmark = pytest.mark.gpu
NT = 8
PRO_NORM, EPI_STORE, EPI_SILU_MUL, EPI_ARGMAX = 1, 0, 2, 3
GENERIC = 16                                                  # mode + 16: the generic kernels
LD_SCRATCH = 18496                                           # the first ld beyond the VALU kernels' LDS bound (18432): attn_batch_gs_kernel.  (The matrix-core kernel moves its rows to the scratch block beyond 512 already)
AM_MAXPOS = 512                                              # BAMD_AM_MAXPOS: the matrix-core kernel keeps its score rows in LDS up to this padded length
N_CTX_SCRATCH = 18560


def assert_cache(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d/%d cells differ, first at %d" % (what, bad.size, got.size, bad[0])


@pytest.fixture(scope="module")
def okats():
    return np.load(os.path.join(GOLDEN, "f64_order_kats.npz"))


@pytest.fixture(scope="module")
def skats():
    return np.load(os.path.join(GOLDEN, "f64_softmax_kats.npz"))


# =====================================================================================================================================================
# RMSNorm sum of squares
# =====================================================================================================================================================
def firing_vector(okats, name):
    """the constructed vector of a length, with the CPU-side proof that the guard fires on it whatever the tree: the sequential mean within 8 units of a
    boundary, and the restated guard firing for it and for three other orders of the same terms"""
    x, eps = okats["x_" + name], float(okats["eps"])
    K = x.size
    o = fs.sum_orders(fs.terms(x))
    assert int(fs.dist_units(fs.mean64(o["seq"], K))) <= fs.NEAR_UNITS and all(fs.guard_fires(s, K) for s in o.values()), name
    return x, eps, K


def quiet_vector(rng, K):
    """a random vector on which NO tree fires: the sequential mean is further from a boundary than the band 2 K + 8 plus the reordering error 2 K"""
    while True:
        x = (rng.standard_normal(K) * 2).astype(np.float32)
        if int(fs.dist_units(fs.mean64(fs.sum_seq(fs.terms(x)), K))) > 4 * K + 8:
            return x


def normed(po, x, w, eps):
    return (po.rms_norm(x, eps) * w).astype(np.float32)


def norm_weights(rng, K):
    return (1 + 0.1 * rng.standard_normal(K)).astype(np.float32)           # random: the weights do not enter the sum


def assert_kernel(bamd, segs, K, epi, mode, kernel):
    tr = booster_amd.trace_matvec([(t, r) for t, _, r in segs], K, PRO_NORM, epi, mode, n_cu=device_cus(bamd))
    assert tr is not None and kernel in tr["kernel"], "the launcher routes the shape elsewhere: %r, wanted %s" % (tr, kernel)


def three_calls(call, want, what):
    for i in range(3):
        assert_bits(call(), want, "%s, call %d" % (what, i))


_QKV = {}


def qkv_weights(po, okats, name, layout):
    """segments [(type, blocks, rows)], norm weights and the oracle's outputs on the constructed vector: built once per (vector, layout)"""
    if (name, layout) not in _QKV:
        x, eps, K = firing_vector(okats, name)
        rng = np.random.default_rng([K] + [v for t, r in layout for v in (t, r)])
        segs = [(t, random_kquant_tensor(t, K, r, rng, amp=4.0), r) for t, r in layout]
        w = norm_weights(rng, K)
        act = normed(po, x, w, eps)
        want = np.concatenate([po.mul_mat_q(t, W, r, K, act, nthreads=NT)[0] for t, W, r in segs])
        _QKV[(name, layout)] = (segs, w, want)
    return _QKV[(name, layout)]


@pytest.mark.parametrize("name,layout,kernel", [
    ("K4096", ((12, 6144),), "matvec_split_mixed_kernelILi12ELi12E"),                   # wq | wk | wv of one type: one segment
    ("K4096", ((12, 5120), (14, 1024)), "matvec_split_mixed_kernelILi12ELi14E"),        # the 8B layout: Q4_K wq | wk, Q6_K wv
    ("K8192", ((12, 10240),), "matvec_split_fast_kernelILi12E"),                        # the 70B row counts: 8192 + 1024 + 1024
])
def test_fused_qkv_fast(bamd, po, okats, name, layout, kernel):
    """the fast split-K QKV kernels (bamd_matvec_fast_b.hip): shared RMSNorm prologue with the wave count as a constant, ring requests in flight across it"""
    x, eps, K = firing_vector(okats, name)
    segs, w, want = qkv_weights(po, okats, name, layout)
    assert_kernel(bamd, segs, K, EPI_STORE, 0, kernel)
    three_calls(lambda: bamd.op_fused_qkv(segs, K, x, w, eps=eps, mode=0), want, "fused QKV %s %r" % (name, layout))


@pytest.mark.parametrize("name,layout,mode,kernel", [
    ("K4096", ((12, 5120), (14, 1024)), 1, "13matvec_kernelILi1ELi0EE"),
    ("K4096", ((12, 5120), (14, 1024)), 2, "19matvec_split_kernelILi1ELi0EE"),
    ("K3072", ((12, 3072), (12, 1024), (14, 1024)), 1, "13matvec_kernelILi1ELi0EE"),     # Llama-3.2-3B QKV rows; K is no power of two: tot / K is a division
    ("K3072", ((12, 3072), (12, 1024), (14, 1024)), 2, "13matvec_kernelILi1ELi0EE"),     # (12 super-blocks do not split over eight waves: mode A again)
    ("K768", ((12, 40),), 1, "13matvec_kernelILi1ELi0EE"),
    ("K768", ((14, 40),), 2, "13matvec_kernelILi1ELi0EE"),
    ("K256", ((12, 64),), 1, "13matvec_kernelILi1ELi0EE"),                               # SMALLK
    ("K256", ((13, 64),), 2, "13matvec_kernelILi1ELi0EE"),
])
def test_generic_kernels(bamd, po, okats, name, layout, mode, kernel):
    x, eps, K = firing_vector(okats, name)
    segs, w, want = qkv_weights(po, okats, name, layout)
    assert_kernel(bamd, segs, K, EPI_STORE, mode + GENERIC, kernel)
    three_calls(lambda: bamd.op_fused_qkv(segs, K, x, w, eps=eps, mode=mode + GENERIC), want, "generic %s %r mode %d" % (name, layout, mode))


@pytest.mark.parametrize("name,t,rows,kernel", [
    ("K4096", 12, 14336, "matvec_gateup7_kernelILi12E"),      # seven pairs per workgroup: waves 4-6 own short pairs, wave 7 helps
    ("K8192", 12, 28672, "matvec_gateup14_kernelILi12E"),     # fourteen pairs: half pairs cross waves through LDS
    ("K8192", 14, 28672, "matvec_gateup14_kernelILi14E"),
    ("K768", 12, 40, "13matvec_kernelILi1ELi2EE"),            # the generic kernel with the SiLU epilogue
])
def test_gate_up(bamd, po, okats, name, t, rows, kernel):
    """every wave of the gate/up kernels passes the prologue (and its fallback barriers) once, before any role waits on a flag"""
    x, eps, K = firing_vector(okats, name)
    rng = np.random.default_rng([5, t, K, rows])
    Wg = random_kquant_tensor(t, K, rows, rng, amp=4.0)
    Wu = random_kquant_tensor(t, K, rows, rng, amp=4.0)
    w = norm_weights(rng, K)
    assert_kernel(bamd, [(t, None, rows), (t, None, rows)], K, EPI_SILU_MUL, 0, kernel)
    act = normed(po, x, w, eps)
    want = po.silu(po.mul_mat_q(t, Wg, rows, K, act, nthreads=NT)[0]) * po.mul_mat_q(t, Wu, rows, K, act, nthreads=NT)[0]
    three_calls(lambda: bamd.op_ffn_gate_up(t, Wg, Wu, rows, K, x, norm_w=w, eps=eps), want, "gate/up type %d %s %d rows" % (t, name, rows))


def test_lm_head_k8192(bamd, po, okats):
    """the fast mode-A lm_head with the arg-max epilogue at K = 8192 (tests/test_gpu_prologue_ring.py has K = 4096): staged prologue, four batch slots"""
    from test_gpu_prologue_ring import argmax_keys
    x, eps, K = firing_vector(okats, "K8192")
    t, rows = 14, 4104                                        # 513 row-groups
    rng = np.random.default_rng([14, K, rows])
    W = random_kquant_tensor(t, K, rows, rng, amp=4.0)
    w = norm_weights(rng, K)
    assert_kernel(bamd, [(t, None, rows)], K, EPI_ARGMAX, 0, "matvec_fast_kernelILi14E")
    want = po.mul_mat_q(t, W, rows, K, normed(po, x, w, eps), nthreads=NT)[0]
    keys = argmax_keys(want)
    for i in range(3):
        got, row = bamd.op_mul_mat_vec_argmax(t, W, rows, K, x, norm_w=w, eps=eps)
        assert_bits(got, want, "lm_head logits K 8192, call %d" % i)
        assert row == int(np.argmax(want)) and argmax_keys(got)[row] == keys.max()


@pytest.mark.parametrize("impl", [0, 2])
def test_quantize_batch(bamd, po, okats, impl):
    """quantize_batch_kernel, T = 3: only token 1 is a constructed vector (a workgroup per token: one takes the fallback between two that do not).
    impl 2 reads the quantiser's f16 record (matrix-core prompt kernel), impl 0 its f32 one"""
    x1, eps, K = firing_vector(okats, "K4096b")
    t, rows = 12, 64
    rng = np.random.default_rng([77, impl])
    X = np.stack([quiet_vector(rng, K), x1, quiet_vector(rng, K)])
    W = random_kquant_tensor(t, K, rows, rng, amp=4.0)
    w = norm_weights(rng, K)
    want = np.stack([po.mul_mat_q(t, W, rows, K, normed(po, X[i], w, eps))[0] for i in range(3)])
    three_calls(lambda: bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=eps, impl=impl), want, "prompt mat-mul with RMSNorm, impl %d" % impl)


def _legacy_family(bamd, po, okats, ref, t, random_tensor, quantize_op, quantize_ref, modes):
    x1, eps, K = firing_vector(okats, "K4096b")
    rng = np.random.default_rng([91, t])
    w = norm_weights(rng, K)
    act = normed(po, x1, w, eps)
    for i in range(3):
        got = quantize_op(x1, norm_w=w, eps=eps)
        assert np.array_equal(got, quantize_ref(act)), "activation blocks, call %d: %d bytes differ" % (i, int((got != quantize_ref(act)).sum()))
    rows = 13                                                  # two row-groups = two workgroups of one busy wave each: seven waves of each have no rows and still owe it the barriers
    W = random_tensor(t, K, rows, rng)
    want = ref.mul_mat(t, W, rows, K, act)
    for mode in modes:                                         # 1: matvec_b32_kernel; 2: matvec_q0_split_kernel (these types have no trace: the mode argument chooses)
        three_calls(lambda: bamd.op_mul_mat_vec(t, W, rows, K, x1, norm_w=w, eps=eps, mode=mode), want, "type %d mat-vec with RMSNorm, mode %d" % (t, mode))
    X = np.stack([quiet_vector(rng, K), x1, quiet_vector(rng, K)])
    want = np.stack([ref.mul_mat(t, W, rows, K, normed(po, X[i], w, eps)) for i in range(3)])
    three_calls(lambda: bamd.op_mul_mat_batch(t, W, rows, K, X, norm_w=w, eps=eps, impl=0), want, "type %d prompt mat-mul with RMSNorm, token 1 constructed" % t)


def test_q8_0_family(bamd, po, okats):
    """ActProQ0::finish_q0 (a textual copy of the fallback): the quantiser op, matvec_b32_kernel<false>, matvec_q0_split_kernel, quantize_batch_b32_kernel<.., false> at T = 3"""
    _legacy_family(bamd, po, okats, lg, lg.Q8_0, random_q0_tensor, bamd.op_quantize_q8_0, lg.quantize_row_q8_0, (1, 2))


def test_q8_1_family(bamd, po, okats):
    """the same with Q8_1 activations: the quantiser op, matvec_b32_kernel<true>, quantize_batch_b32_kernel<.., true> at T = 3 (these types have no split-K kernel)"""
    _legacy_family(bamd, po, okats, l1, l1.Q4_1, random_q1_tensor, bamd.op_quantize_q8_1, l1.quantize_row_q8_1, (1,))


# ---- vectors WITH TEETH (tests/golden/f64_teeth_kats.npz; the cases and both of their expectations: tests/f64_teeth_cases.py) --------------------------
# On K4096b, K256 and K768 above every restated order rounds to the sequential f32: those cases see a hang or a fault of the fallback, not a wrong value.
# On the vectors below the site's own tree rounds to ANOTHER f32 mean and scale, and tests/test_f64_teeth.py proves per case (CPU) that the expected output
# under that mean differs: a kernel that skips the fallback, or sums it wrongly, fails here by value (profiles/f64_guard_paths.txt: a build with
# -DBAMD_NO_F64_GUARD fails every one of them).
@pytest.fixture(scope="module")
def tkats():
    return tc.load()


def run_teeth(bamd, po, tkats, cid):
    """one case of tests/f64_teeth_cases.py: the guard fires on its vector (teeth_vector, CPU), the launcher names the kernel the case names (trace_mv with the
    device's CU count; a matrix-core prompt case: the type's launch counter moves), and three calls give the expectation of the SEQUENTIAL mean bit for bit —
    which is not the expectation of the tree's mean"""
    c = tc.built(po, tkats, cid)
    assert not np.array_equal(c.want_seq.view(np.uint8), c.want_tree.view(np.uint8))
    if c.trace:
        segs, epi, mode, kernel = c.trace
        tr = booster_amd.trace_mv(segs, c.K, PRO_NORM, epi, mode, n_cu=device_cus(bamd))
        assert tr is not None and kernel in tr["kernel"], "the launcher declines or routes the shape elsewhere: %r, wanted %s" % (tr, kernel)
    with tc.switched(bamd, c.switch) if c.switch else contextlib.nullcontext():
        for i in range(3):
            before = bamd.prefill_mfma_runs(c.mfma) if c.mfma is not None else 0
            got = c.run(bamd, c.x, c.w, c.eps)
            what = "%s, call %d" % (cid, i)
            if c.mfma is not None:
                assert bamd.prefill_mfma_runs(c.mfma) == before + 1, what + ": not on the matrix-core kernel"
            if c.argmax:
                from test_gpu_prologue_ring import argmax_keys
                got, row = got
                assert row == int(np.argmax(c.want_seq)) and argmax_keys(got)[row] == argmax_keys(c.want_seq).max(), what + ": row %d" % row
            if c.want_seq.dtype == np.float32:
                assert_bits(got, c.want_seq, what)
            else:
                assert got.dtype == c.want_seq.dtype and np.array_equal(got, c.want_seq), "%s: %d elements differ" % (what, int((got != c.want_seq).sum()))


@pytest.mark.parametrize("cid", [c for c in tc.CASES if c not in tc.FAMILY_IDS and not c.startswith("quantize_batch")])
def test_teeth(bamd, po, tkats, cid):
    """flt_act in its three kernels (matvec_flt_kernel with every epilogue and both activation forms, act_bf16_test_kernel, act_batch_flt_kernel in front of the VALU
    and the matrix-core prompt kernel) and the instantiations of finish_q0 that had no firing vector: the IQ4_NL code objects, the SiLU and arg-max epilogues
    of matvec_b32_kernel (the arg-max's two barriers behind the idle waves' prologue), launches whose first segment has no row-group for a workgroup, and the
    f16 records of quantize_batch_b32_kernel behind the matrix-core prompt kernels"""
    run_teeth(bamd, po, tkats, cid)


@pytest.mark.parametrize("impl", [0, 2])
def test_quantize_batch_teeth(bamd, po, tkats, impl):
    """test_quantize_batch on the vector of ActPro::finish's own tree at K = 4096"""
    run_teeth(bamd, po, tkats, "quantize_batch-q4_k-impl%d" % impl)


@pytest.mark.parametrize("cid", tc.FAMILY["q8_0"] + tc.FAMILY["q8_1"])
def test_legacy_family_teeth(bamd, po, tkats, cid):
    """the steps of test_q8_0_family / test_q8_1_family (the quantiser op, the mat-vec modes, the integer-dot batch; 13 rows) on the vector of finish_q0's own
    tree at K = 4096"""
    run_teeth(bamd, po, tkats, cid)


# =====================================================================================================================================================
# softmax denominator
# =====================================================================================================================================================
class Rows:
    """a micro-batch of T tokens whose token `tf` attends the constructed row `name` on the heads `fire` of KV head `hk` (see the module docstring)"""

    def __init__(self, skats, name, H, Hkv, T, tf, fire, n_ctx, hk=0, seed=0):
        s, self.scale = skats["s_" + name], skats["scale_" + name]
        hd = int(name.split("_hd")[1].split("_")[0])
        valid = int(np.flatnonzero(np.isfinite(s))[-1]) + 1
        gq, Ekv = H // Hkv, Hkv * hd
        pos0 = valid - 1 - tf
        assert pos0 >= 0 and pos0 + T <= n_ctx and all(h // gq == hk for h in fire)
        rng = np.random.default_rng([seed, H, Hkv, T, tf, n_ctx, valid, hd])
        tail = -(rng.random(T - 1 - tf) * 40 + 1).astype(np.float16).astype(np.float32)
        self.S = np.concatenate([s[:valid], tail])                              # the score of every position for q = e_0 (-inf: a masked cell)
        stored = np.where(np.isfinite(self.S), self.S, -1.0).astype(np.float16)
        kc = (rng.standard_normal((n_ctx, Ekv)) * 0.7).astype(np.float16)
        kc[:pos0, hk * hd:(hk + 1) * hd] = 0
        kc[:pos0, hk * hd] = stored[:pos0]
        self.kc = kc.reshape(-1).view(np.uint16).copy()
        self.vc = rng.standard_normal(Ekv * n_ctx).astype(np.float16).view(np.uint16).copy()
        self.c = {h: np.float32(1.0 if h in fire else 0.5) for h in range(hk * gq, (hk + 1) * gq)}
        q = (rng.standard_normal((T, H * hd)) * 2).astype(np.float32)
        for h, c in self.c.items():
            q[:, h * hd:(h + 1) * hd] = 0
            q[:, h * hd] = c
        k = rng.standard_normal((T, Ekv)).astype(np.float32)
        k[:, hk * hd:(hk + 1) * hd] = 0
        k[:, hk * hd] = stored[pos0:pos0 + T]
        self.q, self.k, self.v = q, k, rng.standard_normal((T, Ekv)).astype(np.float32)
        self.rope = np.tile(np.array([1.0, 0.0], np.float32), (n_ctx, hd // 2))  # identity RoPE
        self.H, self.Hkv, self.hd, self.n_ctx, self.pos0, self.T, self.tf, self.fire, self.valid = H, Hkv, hd, n_ctx, pos0, T, tf, set(fire), valid

    def row(self, t, h):
        """the scores of (token t, head h), padded to the token's n_kv with masked entries"""
        n = self.pos0 + t + 1
        pad = min(self.n_ctx, (n + 31) // 32 * 32)
        return np.concatenate([(self.S[:n] * self.c[h]).astype(np.float32), np.full(pad - n, -np.inf, np.float32)])

    def assert_guard(self, po):
        """CPU side: the constructed (token, head) columns fire under every order; every other column of the KV head is further from a boundary than the
        widest band any kernel uses (n = the micro-batch's padded length / 8) plus the reordering error 2 n: it cannot fire"""
        nmax = min(self.n_ctx, (self.pos0 + self.T + 63) // 64 * 64) // 8
        for t in range(self.T):
            for h in self.c:
                r = self.row(t, h)
                den = ss.row_denominators(ss.row_exps(po, r, self.scale))
                d = int(ss.dist(np.array([1.0 / den["seq"]]))[0])
                if t == self.tf and h in self.fire:
                    assert d <= ss.NEAR_UNITS and all(ss.guard_fires(v, r.size) for v in den.values()), "(token %d, head %d) must fire: distance %d" % (t, h, d)
                else:
                    assert d > 4 * nmax + 8, "(token %d, head %d) must not fire: distance %d" % (t, h, d)

    def oracle(self, po, f16_scores):
        kw, vw = self.kc.copy(), self.vc.copy()
        want = po.attention(self.q, self.k, self.v, kw, vw, self.rope, self.H, self.Hkv, self.hd, self.n_ctx, self.pos0, f16_scores)
        # the row the oracle attended IS the constructed one: its output for every firing (token, head), restated from row() — the probabilities of
        # that row (the oracle's soft_max over the micro-batch's padded length) against the V^T rows the oracle left in the cache
        L = po.lib()
        n_kv = min(self.n_ctx, max(32, (self.pos0 + self.T + 31) // 32 * 32))
        for h in self.fire:
            r = self.row(self.tf, h)
            r = np.concatenate([r, np.full(n_kv - r.size, -np.inf, np.float32)])
            live = np.isfinite(r)
            p = po.soft_max(np.where(live, r, 0).astype(np.float32), np.where(live, 0, -np.inf).astype(np.float32), self.scale)
            vt = vw.reshape(self.Hkv * self.hd, self.n_ctx)[(h // (self.H // self.Hkv)) * self.hd:][:self.hd, :n_kv]
            mine = np.array([L.bo_dot_f16_f32_tinyblas(np.ascontiguousarray(vt[d]).ctypes.data, p.ctypes.data, n_kv) for d in range(self.hd)], np.float32)
            assert_bits(want[self.tf, h * self.hd:(h + 1) * self.hd], mine, "the oracle's row of (token %d, head %d) is not the constructed one" % (self.tf, h))
        return want, kw, vw

    def probs(self, po, h):
        """the oracle's probabilities of (the last token, head h)"""
        r = self.row(self.T - 1, h)
        live = np.isfinite(r)
        return po.soft_max(np.where(live, r, 0).astype(np.float32), np.where(live, 0, -np.inf).astype(np.float32), self.scale)


def decode(bamd, po, R, prefill=False, **kw):
    """the single-token op on a one-token Rows against the oracle: output, both caches, and head 0's probabilities where asked for"""
    assert R.T == 1
    R.assert_guard(po)
    want, kw_, vw_ = R.oracle(po, prefill)
    kg, vg = R.kc.copy(), R.vc.copy()
    got = bamd.op_attention(R.q[0], R.k[0], R.v[0], kg, vg, R.rope[R.pos0], R.H, R.Hkv, R.hd, R.n_ctx, R.pos0, prefill_mode=prefill, **kw)
    if kw.get("want_probs"):
        got, gprobs = got
        wprobs = R.probs(po, 0)
        assert_bits(gprobs[:wprobs.size], wprobs, "probabilities of head 0")
    assert_cache(kg, kw_, "K cache"); assert_cache(vg, vw_, "V cache")
    assert_bits(got, want[0], "attention out")


def batch(bamd, po, R, impl, ld=0, scratch=False):
    """the micro-batch op against the oracle.  scratch: whether the kernel the case names keeps its rows in the scratch block — asserted against the
    launcher's own plan (a shape it declines or routes elsewhere fails here)"""
    R.assert_guard(po)
    eff = ld or min((R.pos0 + R.T + 63) // 64 * 64, (R.n_ctx + 63) // 64 * 64)      # the op's own ld: the padded length of the micro-batch's last position
    plan = booster_amd.attention_batch_plan(R.Hkv, R.H // R.Hkv, R.hd, R.T, eff, impl, 0)
    assert plan is not None and plan[1] == 1 and (plan[2] > 0) == scratch, "the launcher routes the shape elsewhere: ld %d, plan %r" % (eff, plan)
    want, kw_, vw_ = R.oracle(po, True)
    kg, vg = R.kc.copy(), R.vc.copy()
    got, _ = bamd.op_attention_batch_ex(R.q, R.k, R.v, kg, vg, R.rope, R.H, R.Hkv, R.hd, R.n_ctx, R.pos0, impl=impl, ld=ld)
    assert_cache(kg, kw_, "K cache"); assert_cache(vg, vw_, "V cache")
    assert_bits(got, want, "attention out, impl %d ld %d" % (impl, ld))


@pytest.mark.parametrize("prefill", [False, True])
@pytest.mark.parametrize("name,H,fire,n_ctx", [("v96_p96_hd128", 4, (2,), 128),       # half a block; only head 2 of four carries the constructed row
                                               ("v64_p64_hd256", 2, (1,), 64)])
def test_fused(bamd, po, skats, name, H, fire, n_ctx, prefill):
    """attn_fused_kernel (the op's default path: one workgroup per query head, rows in LDS)"""
    decode(bamd, po, Rows(skats, name, H, 1, 1, 0, fire, n_ctx), prefill)


@pytest.mark.parametrize("name,n_ctx", [("v96_p96_hd64", 128), ("v4128_p4128_hd64", 4160), ("v8224_p8224_hd64", 8256)])
def test_softmax_kernel(bamd, po, skats, name, n_ctx):
    """attn_softmax_kernel through the three-launch path with the probabilities returned: gq 3 has no softmax + P.V kernel.  Up to 8192 positions the
    exponentials stay in registers (written back for the one lane that redoes the sum), beyond they are in global memory already.  Heads 0 and 2 fire.
    (Routing by the ratio, stated and not asserted: see the module docstring)"""
    decode(bamd, po, Rows(skats, name, 3, 1, 1, 0, (0, 2), n_ctx), want_probs=True)


def test_softmax_kernel_cells(bamd, po, skats):
    """the cell-position path: the masked entries are holes inside the row (free cells), not a tail"""
    R = Rows(skats, "v96_p96_hd64_holes", 3, 1, 1, 0, (0, 2), 128)
    R.assert_guard(po)
    holes = np.flatnonzero(~np.isfinite(R.S))
    assert holes.size >= 4 and holes.max() < R.valid - 1
    cellpos = np.full(R.n_ctx, -1, np.int32); cellpos[:R.valid] = np.arange(R.valid); cellpos[holes] = -1
    kw_, vw_ = R.kc.copy(), R.vc.copy()
    want, wprobs = po.attention_cells(R.q[0], R.k[0], R.v[0], kw_, vw_, R.rope[R.pos0], cellpos, 3, 1, R.hd, R.n_ctx, R.pos0, R.pos0, R.valid)
    assert_bits(wprobs, R.probs(po, 0), "the oracle's row is the constructed one")
    kg, vg = R.kc.copy(), R.vc.copy()
    got, gprobs = bamd.op_attention_cells(R.q[0], R.k[0], R.v[0], kg, vg, R.rope[R.pos0], cellpos, 3, 1, R.hd, R.n_ctx, R.pos0, R.pos0, R.valid)
    assert_cache(kg, kw_, "K cache"); assert_cache(vg, vw_, "V cache")
    assert_bits(gprobs, wprobs, "probabilities of head 0"); assert_bits(got, want, "attention out")


@pytest.mark.parametrize("name,n_ctx", [("v96_p96_hd64", 128), ("v576_p576_hd64", 576)])
@pytest.mark.parametrize("gq,fire", [(2, 1), (4, 3), (8, 6)])
def test_spv(bamd, po, skats, gq, fire, name, n_ctx):
    """attn_spv_kernel<NH>, NH = gq / 2 = 1, 2, 4 heads per workgroup, two workgroups per KV head (spv_launch): the firing head is not the first of its
    workgroup (gq 2: it is the second workgroup's).  (Routing by the ratio and long_path, stated and not asserted: see the module docstring)"""
    assert fire >= gq // 2 and (gq == 2 or fire % (gq // 2) != 0)
    decode(bamd, po, Rows(skats, name, gq, 1, 1, 0, (fire,), n_ctx), long_path=True)


@pytest.mark.parametrize("name,H,T,tf,fire,n_ctx", [
    ("v576_p576_hd128", 4, 4, 2, (1,), 640),                   # token 2 of four: its causal window is the row; gq 4 with one firing head
    ("v80_p96_hd128", 2, 2, 1, (1,), 128),                     # 80 valid positions padded to 96: a masked tail inside the padded length
    ("v96_p96_hd64", 8, 3, 1, (5,), 128),                      # attn_batch_kernel<8>
])
def test_batch_valu(bamd, po, skats, name, H, T, tf, fire, n_ctx):
    """attn_batch_kernel<GQH> (impl 1, gq 2 / 4 / 8: all heads of a KV head in one workgroup, rows in LDS)"""
    batch(bamd, po, Rows(skats, name, H, 1, T, tf, fire, n_ctx), impl=1)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("gq,fire", [(1, 0), (3, 1)])
def test_batch_scratch_rows(bamd, po, skats, gq, fire, hd):
    """attn_batch_gs_kernel<GQ> (impl 1 with ld beyond the LDS bound, on a short sequence): the one lane reads the exponentials from global scratch"""
    batch(bamd, po, Rows(skats, "v96_p96_hd%d" % hd, gq, 1, 3, 1, (fire,), N_CTX_SCRATCH), impl=1, ld=LD_SCRATCH, scratch=True)


MFMA = [(1, (0,)), (2, (1,)), (4, (2,)), (8, (3,)), (4, (1, 2))]     # (gq, firing heads); the last: two firing columns in one workgroup


@pytest.mark.parametrize("name,n_ctx,ld,long", [
    ("v64_p64_hd128", 128, 0, False),                         # LONG = false: one turn of the K ring
    ("v448_p448_hd128", 512, 0, False),                       # LONG = false at the longest padded length that stays in LDS (448 .. 512): several ring turns, 56 .. 64 softmax steps
    ("v576_p576_hd128", 640, 0, True),                        # beyond 512 positions: LONG = true under the op's own ld (576 .. 640)
    ("v64_p64_hd128", N_CTX_SCRATCH, LD_SCRATCH, True),       # LONG = true on a short sequence under a large ld
    ("v576_p576_hd128", N_CTX_SCRATCH, LD_SCRATCH, True),
])
@pytest.mark.parametrize("gq,fire", MFMA)
def test_batch_mfma(bamd, po, skats, gq, fire, name, n_ctx, ld, long):
    """attn_batch_mfma_kernel<GQ, LONG> (impl 2).  LONG = false while the padded length is <= 512: the one lane redoes the sum from LDS; LONG = true
    beyond: from the scratch block behind a pair of fences (the issue's "LONG = false at 576 positions" does not exist: 448 stands in for it).  The
    guard is per COLUMN: one 16-column tile of 16 / gq tokens, the firing column (token 1, or token 5 at gq 1) sits beside columns that do not fire"""
    T = max(2, 16 // gq)
    tf = 5 if gq == 1 else 1
    assert tf * gq + min(fire) > 0 and T <= 16 // gq + 1
    R = Rows(skats, name, gq, 1, T, tf, fire, n_ctx)
    assert ((ld or (R.pos0 + T + 63) // 64 * 64) > AM_MAXPOS) == long
    batch(bamd, po, R, impl=2, ld=ld, scratch=long)


@pytest.mark.parametrize("t,kernel", [(12, "attn_wo_kernel"), (lg.Q8_0, "attn_wo_b32_kernel"), (l1.Q4_1, "attn_wo_b32_kernel")])
def test_colaunch(bamd, po, skats, t, kernel):
    """attention || wo in one launch (attn_fused_body with COLAUNCH = true: what every decode step below 448 positions runs): H 32, Hkv 8, head_dim 128,
    n_ctx 128, position 95, wo 4096 x 4096; head 13 (the second of KV head 3) fires.  x2, the granules, both caches, and the give-up counter"""
    H, Hkv, hd, n_ctx, rows, K = 32, 8, 128, 128, 4096, 4096
    R = Rows(skats, "v96_p96_hd128", H, Hkv, 1, 0, (13,), n_ctx, hk=3)
    R.assert_guard(po)
    tr = booster_amd.trace_attn_wo(H, Hkv, hd, n_ctx, 128, t, rows, K, n_cu=device_cus(bamd))
    sym = kernel + "ILi2E" if t == 12 else "attn_wo_b32_kernelILi2ELi%dE" % t          # head size / 64 = 2; the block-format kernel also by its weight type
    assert kernel in sym and tr is not None and sym in tr["kernel"], "the launcher declines or routes the shape elsewhere: %r" % (tr,)
    rng = np.random.default_rng([3, t])
    W = random_kquant_tensor(t, K, rows, rng) if t == 12 else random_q0_tensor(t, K, rows, rng) if t == lg.Q8_0 else random_q1_tensor(t, K, rows, rng)
    res = rng.standard_normal(rows).astype(np.float32)
    att, kw_, vw_ = R.oracle(po, False)
    att = att[0]
    want = (po.mul_mat_q(t, W, rows, K, att, nthreads=NT)[0] if t == 12 else lg.mul_mat(t, W, rows, K, att) if t == lg.Q8_0 else l1.mul_mat(t, W, rows, K, att)) + res
    kg, vg = R.kc.copy(), R.vc.copy()
    r = bamd.op_attention_wo(R.q[0], R.k[0], R.v[0], kg, vg, R.rope[R.pos0], H, Hkv, hd, n_ctx, R.pos0, t, W, rows, res, lds_ld=128, serial=3, step=96, il=5)
    assert not r["declined"] and r["gave_up"] == 0
    assert np.array_equal((r["gran"] >> np.uint64(32)).astype(np.uint32), np.full(H * hd, tag_of(3, 96, 5), np.uint32)), "granule tags"
    assert_bits((r["gran"] & np.uint64(0xffffffff)).astype(np.uint32).view(np.float32), att, "granule values (attention role)")
    assert_cache(kg, kw_, "K cache"); assert_cache(vg, vw_, "V cache")
    assert_bits(r["x2"], want, "x2 (wo role)")
