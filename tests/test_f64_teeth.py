"""CPU: the constructed RMSNorm vectors WITH TEETH (tests/golden/f64_teeth_kats.npz, gen_f64_teeth_kats.py) and the proof that every GPU case that runs on
one (tests/f64_teeth_cases.py, run by tests/test_gpu_f64_guard.py) can see a wrong sum.  tests/test_f64_order.py's vectors make the guard fire whatever the
tree; on some of them (K256, K768, K4096b) every restated order rounds to the sequential f32, so a kernel that skipped the fallback would still be right.
Here the site's OWN tree — restated from the kernel source in tools/f64_order_search.py — rounds to another f32 mean and another f32 scale, and for every
GPU case the expected output computed with that mean differs from the expected output with the sequential mean in at least one element."""
import os
import sys

import numpy as np
import pytest

import f64_teeth_cases as tc
from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import f64_order_search as fs  # noqa: E402

PAIRS = [("flt", 256), ("flt", 768), ("flt", 3072), ("flt", 4096), ("flt", 8192), ("q0", 768), ("q0", 4096), ("q0", 8192), ("actpro", 4096)]


@pytest.fixture(scope="module")
def tk():
    return tc.load()


def _literal_blocks(t, nwaves=8, batch=4):
    """ActPro::finish / finish_q0 statement by statement, one Python float per lane: issue()'s first batch (blocks wave + b nwaves), then the loop's"""
    nb = t.size // 256
    tot = 0.0
    for wave in range(nwaves):
        lanes = []
        for lane in range(64):
            s = 0.0
            for i0 in range(wave, nb, nwaves * batch):
                for b in range(batch):
                    i = i0 + b * nwaves
                    if i < nb:
                        for c in range(4):
                            s += float(t[i * 256 + lane * 4 + c])
            lanes.append(s)
        tot += fs.wave_sum_f64(np.array(lanes))
    return tot


def _literal_flt(t, nthreads=512):
    """flt_act statement by statement: for (k4 = threadIdx.x; k4 < n4; k4 += blockDim.x)"""
    part = []
    for th in range(nthreads):
        s = 0.0
        for k4 in range(th, t.size // 4, nthreads):
            for c in range(4):
                s += float(t[4 * k4 + c])
        part.append(s)
    tot = 0.0
    for w in range(nthreads // 64):
        tot += fs.wave_sum_f64(np.array(part[w * 64:(w + 1) * 64]))
    return tot


def test_restated_trees():
    """the vectorised trees of tools/f64_order_search.py against the kernels' loops written out thread by thread; the generalised ActPro::finish /
    finish_q0 tree is sum_tree at K = 4096; wave_sum_f64 adds every lane once"""
    rng = np.random.default_rng(3)
    for K in (256, 768, 3072, 4096, 8192):
        t = fs.terms((rng.standard_normal(K) * np.exp(rng.standard_normal(K) * 2.0)).astype(np.float32))
        assert fs.sum_tree_blocks(t) == _literal_blocks(t) and fs.sum_tree_flt(t) == _literal_flt(t)
        for tree in (fs.sum_tree_blocks, fs.sum_tree_flt):
            assert abs(tree(t) - fs.sum_seq(t)) <= 2 * K * 2.0 ** -53 * fs.sum_seq(t)
        if K == fs.K:
            assert fs.sum_tree_blocks(t) == fs.sum_tree(t)
    for lane in range(64):
        one = np.zeros(64); one[lane] = 1.0
        assert fs.wave_sum_f64(one) == 1.0
    assert fs.wave_sum_f64(np.arange(64.0)) == 2016.0


def test_fixture_holds_every_pair(tk):
    assert {n[2:] for n in tk.files if n.startswith("x_")} == {"%s_%d" % p for p in PAIRS}
    assert tk["eps"] == np.float32(1e-5)


@pytest.mark.parametrize("site,K", PAIRS)
def test_vector_has_teeth(tk, po, site, K):
    """(a) - (d) of the generator from the stored bytes (teeth_vector asserts them), the stored means, and the oracle's RMSNorm = the sequential mean"""
    x, eps, m_seq, m_tree = tc.teeth_vector(tk, site, K)
    assert x.dtype == np.float32 and abs(int(m_seq.view(np.uint32)) - int(m_tree.view(np.uint32))) == 1
    assert np.array_equal(po.rms_norm(x, eps).view(np.uint32), (x * fs.scale32(m_seq, eps)).astype(np.float32).view(np.uint32))
    assert not np.array_equal(po.rms_norm(x, eps).view(np.uint32), (x * fs.scale32(m_tree, eps)).astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("site,K", PAIRS)
def test_normed_with_mean_is_the_oracle(tk, po, site, K):
    x, eps, m_seq, _ = tc.teeth_vector(tk, site, K)
    w = tc.norm_weights(np.random.default_rng(K), K)
    assert np.array_equal(tc.normed_with_mean(x, w, m_seq, eps).view(np.uint32), (po.rms_norm(x, eps) * w).astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("cid", list(tc.CASES))
def test_tree_mean_changes_the_expected_output(tk, po, cid):
    """what makes a skipped or wrong fallback visible on the GPU: the case's expectation under the tree's mean is another one.  (A case whose outputs happen
    to agree takes the next seed of its pair: SKIP in gen_f64_teeth_kats.py.)"""
    c = tc.built(po, tk, cid)
    assert c.want_seq.shape == c.want_tree.shape and c.want_seq.dtype == c.want_tree.dtype
    if c.want_seq.dtype == np.float32:
        assert np.isfinite(c.want_seq).all() and np.isfinite(c.want_tree).all()
    differ = int((c.want_seq.view(np.uint8) != c.want_tree.view(np.uint8)).sum())
    assert differ > 0, "%s: pair (%s, %d) needs its next seed" % (cid, c.site, c.K)
    if c.batch:                                                                   # only token 1 is constructed
        assert np.array_equal(c.want_seq[0], c.want_tree[0]) and np.array_equal(c.want_seq[2], c.want_tree[2])
    if c.argmax:
        assert np.flatnonzero(c.want_seq == c.want_seq.max()).size == 1            # the chosen row is unambiguous


def test_case_kernels_are_named():
    """every mat-vec case names its kernel and the launcher agrees (bamd_trace_mv is host only): the three kernels that inline flt_act's sum and the
    finish_q0 instantiations of the issue"""
    import booster_amd
    kernels = set()
    for cid, (site, K, batch, f) in tc.CASES.items():
        c = f(None, np.random.default_rng(0), K)
        if c.get("trace"):
            segs, epi, mode, kernel = c["trace"]
            tr = booster_amd.trace_mv(segs, K, tc.PRO_NORM, epi, mode)
            assert tr is not None and kernel in tr["kernel"], "%s: %r, wanted %s" % (cid, tr, kernel)
            kernels.add(kernel)
    for want in ("matvec_flt_kernelILb0ELi1ELi0E", "matvec_flt_kernelILb1ELi1ELi2E", "matvec_flt_kernelILb1ELi1ELi3E", "matvec_b32_nl_kernelILb0ELi1ELi0E",
                 "matvec_b32_nl_kernelILb0ELi1ELi2E", "matvec_b32_nl_kernelILb0ELi1ELi3E", "matvec_b32_kernelILb0ELi1ELi2E", "matvec_b32_kernelILb1ELi1ELi2E",
                 "matvec_b32_kernelILb0ELi1ELi3E", "matvec_b32_kernelILb1ELi1ELi3E", "matvec_q0_split_kernelILi1ELi0E"):
        assert want in kernels, want


def test_generator_reproduces_the_fixture(tk):
    """fixed seeds: the search of a pair gives the stored vector again (one pair here, about a second; the whole file is a minute of the generator)"""
    sys.path.insert(0, GOLDEN)
    import gen_f64_teeth_kats as gen
    assert [(s, k) for s, ks in gen.PAIRS for k in ks] == PAIRS and gen.EPS == tk["eps"]
    x, m_seq, m_tree, seed = gen.find("flt", 0, 3072)
    assert seed == int(tk["seed_flt_3072"]) and np.array_equal(x.view(np.uint32), tk["x_flt_3072"].view(np.uint32))
    assert m_seq == tk["mean_seq_flt_3072"] and m_tree == tk["mean_tree_flt_3072"]
