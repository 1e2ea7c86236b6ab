"""CPU: the oracle's cell model (bo_kv_seq_rm / _add / _div, the K-shift and find_slot inside bo_decode) replays the committed reference fixtures
of context shift and Self-Extend step by step, through the same scripts as tests/test_gpu_fullsize_ref.py; and its op-level functions of the
shifted path (bo_k_shift, bo_attention_cells), which tests/test_gpu_shift.py holds the HIP kernels to, are checked against independent
restatements: bo_k_shift against numpy's f32 arithmetic of ggml_compute_forward_rope_f16 on bo_rope_cache rows, and bo_attention_cells with cells
that still follow positions against bo_attention."""
import os

import numpy as np
import pytest

from booster_amd import gguf
from goldenio import load_bgld
from refmodel import FULLSIZE, check_step, load_fixture, model_for, prompt_of

gen = FULLSIZE.gen


def _oracle_ctx(po, cfg):
    fx = load_fixture(FULLSIZE, cfg)
    g = load_bgld(FULLSIZE.fixture_path(cfg))
    _, n_prompt, n_decode, n_ctx = FULLSIZE.shape(cfg)
    om = po.OracleModel(gguf.GGUFReader(model_for(FULLSIZE, cfg, fx)))
    return fx, g, om, po.OracleContext(om, n_ctx, nthreads=min(8, os.cpu_count() or 1)), n_prompt, n_decode, n_ctx


# the fixtures of the shifted path that the oracle can replay (it has no YaRN: shift_yarn is checked on the GPU only), with their recorded events
SHIFTS = {"shift": 3, "shift_hd128": 2}
WINDOWS = {"selfextend": 6, "selfextend_gq8": 3}


@pytest.mark.parametrize("cfg", sorted(SHIFTS))
def test_oracle_context_shift_replays_reference(po, cfg):
    """the script of test_context_shift_matches_reference on the oracle: every step's token, probe logits, top logit and all-logit digest,
    n_past of every step and the steps of the shifts as the reference recorded them"""
    fx, g, om, oc, n_prompt, n_decode, n_ctx = _oracle_ctx(po, cfg)
    n_keep = gen.N_KEEP[cfg]
    prompt = prompt_of(n_prompt, om.V)
    check_step(fx, 0, oc.decode(prompt, 0), "oracle %s prompt" % cfg)
    n_past, shifts = n_prompt, []
    for s in range(n_decode):
        if n_past + 1 > n_ctx:
            n_past = oc.context_shift(n_keep, n_past)
            shifts.append(s)
        assert n_past == int(g["n_past_of_step"][s])
        lg = oc.decode([int(fx["tokens"][s])], n_past); n_past += 1
        check_step(fx, s + 1, lg, "oracle %s decode (after %d shifts)" % (cfg, len(shifts)))
    assert shifts == [int(x) for x in g["shift_steps"]] and len(shifts) == SHIFTS[cfg]
    oc.close()


@pytest.mark.parametrize("cfg", sorted(WINDOWS))
def test_oracle_self_extend_replays_reference(po, cfg):
    """the script of test_self_extend_matches_reference on the oracle (cpp/bridge.cpp:509-522): every step against the reference's record"""
    fx, g, om, oc, n_prompt, n_decode, n_ctx = _oracle_ctx(po, cfg)
    ga_n, ga_w = (-gen.N_KEEP[cfg]) // 100, (-gen.N_KEEP[cfg]) % 100
    prompt = prompt_of(n_prompt, om.V)
    check_step(fx, 0, oc.decode(prompt, 0), "oracle %s prompt" % cfg)
    n_past, ga_i, events = n_prompt, 0, []
    for s in range(n_decode):
        while n_past >= ga_i + ga_w:
            ib, bd = (ga_n * ga_i) // ga_w, (ga_w // ga_n) * (ga_n - 1)
            dd = (ga_w // ga_n) - ib * bd - ga_w
            oc.kv_seq_add(ga_i, n_past, ib * bd)
            oc.kv_seq_div(ga_i + ib * bd, ga_i + ib * bd + ga_w, ga_n)
            oc.kv_seq_add(ga_i + ib * bd + ga_w, n_past + ib * bd, dd)
            n_past -= bd
            ga_i += ga_w // ga_n
            events.append(s)
        assert n_past == int(g["n_past_of_step"][s])
        lg = oc.decode([int(fx["tokens"][s])], n_past); n_past += 1
        check_step(fx, s + 1, lg, "oracle %s decode (after %d windows)" % (cfg, len(events)))
    assert events == [int(x) for x in g["shift_steps"]] and len(events) == WINDOWS[cfg]
    oc.close()


def rope_f16_numpy(po, kc, n_ctx, Hkv, hd, delta, **rope):
    """ggml.c:14249-14262 per cell: x0, x1 from f16, x0*cos - x1*sin and x0*sin + x1*cos as separate f32 operations, round to f16"""
    x = kc.view(np.float16).astype(np.float32).reshape(n_ctx, Hkv, hd // 2, 2)
    cs = np.stack([po.rope_cache(int(d), hd, **rope) for d in delta]).reshape(n_ctx, 1, hd // 2, 2)
    c, s = cs[..., 0], cs[..., 1]
    x0, x1 = x[..., 0], x[..., 1]
    with np.errstate(over="ignore"):
        out = np.stack([(x0 * c) - (x1 * s), (x0 * s) + (x1 * c)], axis=-1).astype(np.float16)
    return out.reshape(-1).view(np.uint16)


@pytest.mark.parametrize("Hkv,hd", [(2, 64), (3, 128), (1, 256)])
@pytest.mark.parametrize("rope", [dict(freq_base=500000.0), dict(freq_base=10000.0, freq_scale=0.25, ext_factor=1.0, attn_factor=1.25, n_ctx_orig=64)])
def test_k_shift_is_rope_f16(po, Hkv, hd, rope):
    n_ctx = 96
    rng = np.random.default_rng(hd + Hkv)
    kc = (rng.standard_normal(n_ctx * Hkv * hd) * 0.7).astype(np.float16).view(np.uint16)
    kc = kc.reshape(n_ctx, -1).copy()
    kc[::5, 0] = 0x0000; kc[::5, 1] = 0x8000                                             # (+0, -0)
    kc[1::5, 2:4] = 0x7bff                                                               # 65504: overflows
    kc[2::5, 4:8] = [0x0001, 0x83ff, 0x0400, 0x8002]                                     # subnormals
    kc = kc.reshape(-1)
    delta = rng.integers(-32768, 32769, n_ctx).astype(np.int32)
    delta[::3] = 0
    got = po.k_shift(kc, n_ctx, Hkv, hd, delta, rope.get("freq_base"), rope.get("freq_scale", 1.0), None, rope.get("ext_factor", 0.0),
                     rope.get("attn_factor", 1.0), rope.get("n_ctx_orig", 8192))
    want = rope_f16_numpy(po, kc, n_ctx, Hkv, hd, delta, **rope)
    assert np.array_equal(got, want)
    assert (got.reshape(n_ctx, -1)[::15, 1] == 0x0000).all()                             # zero-delta cells are rotated too: -0 -> +0


@pytest.mark.parametrize("H,Hkv,hd", [(8, 2, 64), (6, 2, 128), (4, 1, 256)])
def test_attention_cells_follows_positions(po, H, Hkv, hd):
    """cells that still follow positions (cell i holds i, the rest free): bo_attention_cells == bo_attention's T == 1 path, bit for bit"""
    n_ctx = 160
    rng = np.random.default_rng(H * hd)
    Ekv = Hkv * hd
    for pos in (0, 31, 70, 159):
        kc = (rng.standard_normal(n_ctx * Ekv) * 0.7).astype(np.float16).view(np.uint16).copy()
        vc = rng.standard_normal(Ekv * n_ctx).astype(np.float16).view(np.uint16).copy()
        q = (rng.standard_normal(H * hd) * 2).astype(np.float32)
        k = rng.standard_normal(Ekv).astype(np.float32)
        v = rng.standard_normal(Ekv).astype(np.float32)
        rope = po.rope_cache(pos, hd, 500000.0)
        kc2, vc2 = kc.copy(), vc.copy()
        want = po.attention(q, k, v, kc2, vc2, rope, H, Hkv, hd, n_ctx, pos, False)[0]
        cp = np.where(np.arange(n_ctx) <= pos, np.arange(n_ctx), -1).astype(np.int32)
        n_kv = min(n_ctx, max(32, (pos + 1 + 31) // 32 * 32))
        got, probs = po.attention_cells(q, k, v, kc, vc, rope, cp, H, Hkv, hd, n_ctx, pos, pos, n_kv)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "pos %d" % pos
        assert np.array_equal(kc, kc2) and np.array_equal(vc, vc2)
        assert probs.size == n_kv and (probs[pos + 1:] == 0).all() and abs(float(probs.sum()) - 1.0) < 1e-5
