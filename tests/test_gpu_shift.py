"""GPU: the path the engine switches to after position edits (bamd_kv_seq_rm / _add / _div: Booster's context shift and Self-Extend), at op level
against the CPU oracle, bit for bit:

  K-shift           bamd_op_k_shift = k_shift_table (the engine's delta -> (cos, sin) table, shared with kv_update) + k_shift_kernel over the
                    chain-major cache, against bo_k_shift (ggml_compute_forward_rope_f16 over every cell, llama.cpp:8482-8512)
  shifted cells     bamd_op_attention_cells = step_begin_kernel (cell / n_kv from cell_plus1 / n_kv_fixed, the rope_cur row) + the cellpos entry of
                    the token written as bamd_stage_step writes it + attn_qk_kernel<G, LG, SH = true> + softmax / P.V, against bo_attention_cells
                    (the reference's mask by the position each cell holds, llama.cpp:14152-14200)

Every cell map and every value edge a case is meant to reach is asserted to occur, so a generator change cannot quietly drop one."""
import math

import numpy as np
import pytest

from bitcheck import assert_bits

pytestmark = pytest.mark.gpu


def assert_f16(got, want, what):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d/%d f16 values differ, first at %d: %#06x vs %#06x" % (what, bad.size, got.size, bad[0], got.flat[bad[0]], want.flat[bad[0]])


def llama3_rope_freqs(hd, base=500000.0, factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0, orig_ctx=8192):
    """rope_freqs.weight as the Llama-3.1 conversion computes it (rope scaling type "llama3")"""
    out = []
    for i in range(0, hd, 2):
        freq = 1.0 / (base ** (i / hd))
        wavelen = 2 * math.pi / freq
        if wavelen < orig_ctx / high_freq_factor:
            out.append(1.0)
        elif wavelen > orig_ctx / low_freq_factor:
            out.append(factor)
        else:
            smooth = (orig_ctx / wavelen - low_freq_factor) / (high_freq_factor - low_freq_factor)
            out.append(1.0 / ((1 - smooth) / factor + smooth))
    return np.array(out, np.float32)


# (name, freq_base, freq_scale, llama3 freq factors, ext_factor, attn_factor, n_ctx_orig)
ROPES = [("theta5e5", 500000.0, 1.0, False, 0.0, 1.0, 8192),
         ("theta1e4", 10000.0, 1.0, False, 0.0, 1.0, 8192),
         ("llama3_freqs", 500000.0, 1.0, True, 0.0, 1.0, 8192),
         ("freq_scale_0.25", 10000.0, 0.25, False, 0.0, 1.0, 8192),
         ("yarn", 10000.0, 0.25, False, 1.0, 1.25, 64)]


def delta_maps(n_ctx, rng):
    """the delta maps of a K-shift: {name: delta[n_ctx]}"""
    n_keep = 4
    nd = (n_ctx - n_keep) // 2
    shift = np.zeros(n_ctx, np.int32); shift[n_keep + nd:] = -nd                        # Booster's context shift: one value on a range
    se = np.zeros(n_ctx, np.int32)                                                       # Self-Extend-like: seq_div by 4 over a window, then a seq_add
    w0, w1 = n_ctx // 8, n_ctx // 8 + min(n_ctx // 2, 512)
    p = np.arange(n_ctx)
    se[w0:w1] = (p[w0:w1] // 4) - p[w0:w1]
    se[w1:] = (w1 // 4) - w1 - 7
    rnd = rng.integers(-32768, 32769, n_ctx).astype(np.int32)                            # random deltas in [-32768, 32768] ...
    rnd[rng.choice(n_ctx, max(4, n_ctx // 16), replace=False)] = 0                      # ... with zero cells among them
    return {"shift": shift, "selfextend": se, "random": rnd, "zero": np.zeros(n_ctx, np.int32)}


def k_values(n_ctx, Hkv, hd, rng):
    """a seeded normal * 0.7 K cache (f16 bits, reference layout) with edge rows: (+0, -0) pairs, f16 subnormals, +-65504 pairs"""
    kc = (rng.standard_normal(n_ctx * Hkv * hd) * 0.7).astype(np.float16).view(np.uint16).reshape(n_ctx, Hkv * hd).copy()
    for c in range(0, n_ctx, 7):                                                         # (+0, -0): the reference's x0*c - x1*s turns -0 into +0
        kc[c, 0:8:2] = 0x0000; kc[c, 1:8:2] = 0x8000
    for c in range(3, n_ctx, 11):                                                        # f16 subnormals (and small normals rotated into them)
        kc[c, 8:24] = rng.integers(1, 0x400, 16).astype(np.uint16) | (rng.integers(0, 2, 16).astype(np.uint16) << 15)
        kc[c, 24:32] = np.array([0x0400, 0x8400, 0x0401, 0x0402, 0x83ff, 0x0001, 0x8001, 0x03ff], np.uint16)
    for c in range(5, n_ctx, 13):                                                        # +-65504 pairs: the rotation overflows to +-inf
        kc[c, 32:40] = np.array([0x7bff, 0xfbff, 0x7bff, 0x7bff, 0xfbff, 0xfbff, 0xfbff, 0x7bff], np.uint16)
    return kc.reshape(-1)


def is_sub16(u):
    return ((u & 0x7c00) == 0) & ((u & 0x03ff) != 0)


def is_inf16(u):
    return (u & 0x7fff) == 0x7c00


def run_k_shift_cases(bamd, po, Hkv, hd, n_ctx, seed):
    rng = np.random.default_rng(seed)
    kc = k_values(n_ctx, Hkv, hd, rng)
    reached = dict(zero_pair=False, sub_in=bool(is_sub16(kc).any()), sub_out=False, inf=False)
    for rname, base, fscale, llama3, ext, attn, orig in ROPES:
        ff = llama3_rope_freqs(hd) if llama3 else None
        for dname, delta in delta_maps(n_ctx, rng).items():
            want = po.k_shift(kc, n_ctx, Hkv, hd, delta, base, fscale, ff, ext, attn, orig)
            got = bamd.op_k_shift(kc, n_ctx, Hkv, hd, delta, base, fscale, ff, ext, attn, orig)
            what = "K-shift Hkv %d hd %d n_ctx %d rope %s deltas %s" % (Hkv, hd, n_ctx, rname, dname)
            assert not np.isnan(want.view(np.float16)).any(), what + ": the oracle produced a NaN from finite inputs"
            assert_f16(got, want, what)
            k2, w2 = kc.reshape(n_ctx, -1), want.reshape(n_ctx, -1)
            z = np.flatnonzero(delta == 0)
            if z.size:                                                                   # a -0 in a zero-delta cell comes out +0
                zc = z[z % 7 == 0]
                if zc.size and (k2[zc, 1] == 0x8000).all() and (w2[zc, 1] == 0x0000).all():
                    reached["zero_pair"] = True
            reached["sub_out"] |= bool(is_sub16(want).any())
            reached["inf"] |= bool(is_inf16(want).any())
    assert all(reached.values()), "edges not reached: %r" % reached


@pytest.mark.parametrize("Hkv,hd", [(1, 64), (3, 64), (2, 128), (8, 128), (32, 128), (8, 256), (2, 192), (1, 256)])
@pytest.mark.parametrize("n_ctx", [96, 640])
def test_k_shift(bamd, po, Hkv, hd, n_ctx):
    """k_shift_kernel + the engine's table code == bo_k_shift over the whole cache: (32, 128) has 2048 pairs per cell (two passes of the kernel's
    strided loop), (8, 256) exactly 1024; context-shift, Self-Extend-like, random and all-zero delta maps under five rope settings (YaRN: even the
    zero-delta cells are scaled by mscale)"""
    run_k_shift_cases(bamd, po, Hkv, hd, n_ctx, 1000 * Hkv + hd + n_ctx)


def test_k_shift_long_context(bamd, po):
    run_k_shift_cases(bamd, po, 8, 128, 8192, 8192)


# ---- shifted-cell attention ------------------------------------------------------------------------------------------------------------
def pad32(n):
    return (n + 31) // 32 * 32


def n_kv_of(cellpos, n_ctx):
    used = np.flatnonzero(cellpos >= 0)
    return min(n_ctx, max(32, pad32(int(used.max()) + 1)))                               # llama.cpp:14693-14701


def cell_maps(n_ctx, rng):
    """(name, cellpos with the token's cell already holding pos, cell, pos, n_kv) of the situations the shifted path meets"""
    out = []
    n_keep = 4
    # after a context shift of a full cache: cells [n_keep, n_keep + nd) were freed and refilled in cell order with the NEWEST positions
    nd = (n_ctx - n_keep) // 2
    cp = np.arange(n_ctx, dtype=np.int32); cp[n_keep + nd:] -= nd; cp[n_keep:n_keep + nd] = -1
    m = int(rng.integers(1, nd))
    first = n_ctx - nd
    cp[n_keep:n_keep + m] = first + np.arange(m)
    cell, pos = n_keep + m, first + m
    cp[cell] = pos
    assert cp[n_keep:cell].min() > cp[n_keep + nd:].max()
    out.append(("context_shift", cp, cell, pos, n_kv_of(cp, n_ctx)))
    # the first token right after the shift: the hole starts at the token's cell, a half-filled cache behind it
    cp = np.arange(n_ctx, dtype=np.int32); cp[n_keep + nd:] -= nd; cp[n_keep:n_keep + nd] = -1
    cell, pos = n_keep, n_ctx - nd
    cp[cell] = pos
    assert cell < pos
    out.append(("after_shift_first", cp, cell, pos, n_kv_of(cp, n_ctx)))
    # after Self-Extend: positions divided by 4 over a window, duplicated and far below the cell index
    used = n_ctx - n_ctx // 4
    cp = np.full(n_ctx, -1, np.int32)
    p = np.arange(used)
    w0 = n_ctx // 8
    cp[:used] = np.where(p < w0, p, w0 + (p - w0) // 4)
    cell = used; pos = int(cp[:used].max()) + 1
    cp[cell] = pos
    assert np.unique(cp[w0:used]).size < used - w0 and cp[used - 1] < (used - 1) // 2
    out.append(("selfextend", cp, cell, pos, n_kv_of(cp, n_ctx)))
    # free cells inside [0, n_kv), including the last half block; n_kv % 64 == 32 where the context allows it
    n_kv = n_ctx - 32 if (n_ctx - 32) % 64 == 32 else n_ctx
    cp = np.arange(n_ctx, dtype=np.int32); cp[n_kv:] = -1
    holes = rng.choice(n_kv - 1, n_kv // 5, replace=False)
    cp[holes] = -1
    cp[n_kv - 20:n_kv - 5] = -1                                                          # inside the last half block
    cp[n_kv - 1] = n_kv - 1
    cell, pos = int(holes[0]), n_kv - 10                                                 # the token takes a former hole, at a freed position below later ones
    cp[cell] = pos
    assert (cp[:n_kv] == -1).any() and (cp[n_kv - 32:n_kv] == -1).any() and (cp[:n_kv] > pos).any() and n_kv % 64 == 32
    out.append(("holes", cp, cell, pos, n_kv))
    # cells below n_kv that hold positions > pos (a scrambled cache), the token's cell > pos
    cp = rng.permutation(n_ctx).astype(np.int32)
    pos = n_ctx // 3
    cell = int(np.flatnonzero(np.arange(n_ctx) > pos)[0] + n_ctx // 4)
    cp[cp == pos] = cp[cell]; cp[cell] = pos
    assert (cp[:n_kv_of(cp, n_ctx)] > pos).any() and cell > pos
    out.append(("later_positions", cp, cell, pos, n_kv_of(cp, n_ctx)))
    # the token at the last cell, n_ctx - 1, with a position far below it
    cp = np.arange(n_ctx, dtype=np.int32) // 2
    cell = n_ctx - 1; pos = int(cp[cell - 1]) + 1
    cp[cell] = pos
    out.append(("last_cell", cp, cell, pos, n_ctx))
    # n_kv = n_ctx while pos < 64: a few early positions spread over the whole cache
    cp = np.full(n_ctx, -1, np.int32)
    spots = np.sort(rng.choice(n_ctx - 1, 40, replace=False))
    cp[spots] = np.arange(40)
    cp[n_ctx - 1] = 40
    cell = int(np.flatnonzero(cp < 0)[3]); pos = 41
    cp[cell] = pos
    assert n_kv_of(cp, n_ctx) == n_ctx and pos < 64
    out.append(("full_n_kv_small_pos", cp, cell, pos, n_ctx))
    return out


def run_cells_cases(bamd, po, H, Hkv, hd, n_ctx, seed, tiles=0, maps=None):
    rng = np.random.default_rng(seed)
    Ekv = Hkv * hd
    kc = (rng.standard_normal(n_ctx * Ekv) * 0.7).astype(np.float16).view(np.uint16).copy()
    vc = rng.standard_normal(Ekv * n_ctx).astype(np.float16).view(np.uint16).copy()
    seen = set()
    for name, cp, cell, pos, n_kv in (maps or cell_maps(n_ctx, rng)):
        assert cp[cell] == pos and 0 <= cell < n_kv <= n_ctx and pos < n_ctx
        q = (rng.standard_normal(H * hd) * 2).astype(np.float32)
        k = rng.standard_normal(Ekv).astype(np.float32)
        v = rng.standard_normal(Ekv).astype(np.float32)
        rope = po.rope_cache(pos, hd, 500000.0)
        kc2, vc2 = kc.copy(), vc.copy()
        want, wprobs = po.attention_cells(q, k, v, kc2, vc2, rope, cp, H, Hkv, hd, n_ctx, pos, cell, n_kv, nthreads=16)
        gcp = cp.copy(); gcp[cell] = -1                                                  # the op writes the token's entry itself
        got, gprobs = bamd.op_attention_cells(q, k, v, kc, vc, rope, gcp, H, Hkv, hd, n_ctx, pos, cell, n_kv, tiles=tiles)
        what = "cells %s H %d Hkv %d hd %d n_ctx %d cell %d pos %d n_kv %d" % (name, H, Hkv, hd, n_ctx, cell, pos, n_kv)
        assert np.array_equal(kc, kc2) and np.array_equal(vc, vc2), what + ": KV store differs"
        assert_bits(gprobs, wprobs, what + ": head 0 probabilities")
        assert_bits(got, want, what + ": attention out")
        seen.add(name)
    return seen


CELL_SHAPES = [(8, 8, 64), (4, 2, 64), (6, 2, 128), (8, 2, 128), (10, 2, 128), (12, 2, 192), (7, 1, 256), (8, 1, 128), (4, 1, 256),
               (2, 1, 128), (16, 2, 64), (3, 1, 192)]


@pytest.mark.parametrize("H,Hkv,hd", CELL_SHAPES)
@pytest.mark.parametrize("n_ctx", [96, 640, 4096])
def test_attention_cells(bamd, po, H, Hkv, hd, n_ctx):
    """attn_qk_kernel<G, LG, true> for gq 1-8 x head_dim 64-256 + the softmax / P.V behind it == bo_attention_cells: after a context shift, after
    Self-Extend, holes in [0, n_kv), cells holding later positions, the token in a former hole / beyond its position / at the last cell"""
    seen = run_cells_cases(bamd, po, H, Hkv, hd, n_ctx, 7 * H + 31 * hd + n_ctx)
    assert seen == {"context_shift", "after_shift_first", "selfextend", "holes", "later_positions", "last_cell", "full_n_kv_small_pos"}


def test_attention_cells_softmax_pv_pair(bamd, po):
    """gq 4 x 128 at n_ctx 20480 with n_kv > 16 384: the score kernel's later prefetch batches, the softmax + P.V pair (score rows beyond the LDS)"""
    n_ctx = 20480
    rng = np.random.default_rng(20480)
    maps = []
    for name, cp, cell, pos, n_kv in cell_maps(n_ctx, rng):
        if n_kv > 16384:
            maps.append((name, cp, cell, pos, n_kv))
    assert len(maps) >= 4
    run_cells_cases(bamd, po, 4, 1, 128, n_ctx, 20481, maps=maps)


@pytest.mark.parametrize("H,Hkv,hd", [(8, 2, 128), (6, 2, 128), (8, 1, 256)])
def test_attention_cells_one_tile_workgroup(bamd, po, H, Hkv, hd):
    """tiles = 1 (BAMD_QK_TILES=1): ONE score workgroup per KV head loops over all 16 tiles of a 1024-cell context in batches"""
    seen = run_cells_cases(bamd, po, H, Hkv, hd, 1024, 1024 + H + hd, tiles=1)
    assert len(seen) == 7


# ---- whole models against the oracle's cell model ----------------------------------------------------------------------------------------
MODELS = {"gq3_hd128": dict(E=768, H=6, Hkv=2, rope_freqs=True), "gq4_hd256": dict(E=1024, H=4, Hkv=1),
          "gq2_hd192": dict(E=768, H=4, Hkv=2), "gq1_hd64": dict(E=512, H=8, Hkv=8)}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def open_pair(bamd, po, tmp_path, name, n_ctx):
    from booster_amd import gguf
    p = str(tmp_path / (name + ".gguf"))
    gguf.write_synthetic_llama(p, L=2, F=768, V=512, theta=500000.0, seed=41, **MODELS[name])
    om = po.OracleModel(gguf.GGUFReader(p)); oc = po.OracleContext(om, n_ctx, nthreads=16)
    m = bamd.Model(p); ctx = bamd.Context(m, n_ctx)
    return om, oc, m, ctx


def same_logits(lg_g, lg_o, what):
    assert np.array_equal(bits(lg_g), bits(lg_o)), "%s: logits differ, max |d| = %g" % (what, np.abs(lg_g - lg_o).max())


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("n_ctx", [96, 640])
def test_model_context_shift_vs_oracle(bamd, po, tmp_path, name, n_ctx):
    """a prompt of n_ctx / 2 tokens, then greedy steps past n_ctx with Booster's context shift (n_keep 4) on both sides until two shifts have
    happened and 8 steps more: every step's logits bit for bit.  gq4_hd256 at n_ctx 96 runs bamd_generate_greedy (device-side loop over cells)
    from the first shift to the second; gq2_hd192 at n_ctx 96 then truncates with kv_seq_rm(n_keep, -1), which brings the cells back to
    "cell i holds position i", and evaluates a 20-token micro-batch on the batched kernels"""
    om, oc, m, ctx = open_pair(bamd, po, tmp_path, name, n_ctx)
    n_keep = 4
    prompt = [(7919 * i + 13) % 512 for i in range(n_ctx // 2)]
    lg_o = oc.decode(prompt, 0); same_logits(ctx.decode(prompt, 0), lg_o, "prompt")
    n_past, shifts, s, greedy_done = len(prompt), 0, 0, False
    while shifts < 2 or s < 8:
        if n_past + 1 > n_ctx:
            old = n_past
            n_past = ctx.context_shift(n_keep, old)
            assert oc.context_shift(n_keep, old) == n_past
            shifts += 1; s = 0
        t = int(np.argmax(lg_o))
        if name == "gq4_hd256" and n_ctx == 96 and shifts == 1 and not greedy_done:
            K = n_ctx - n_past
            toks = [t]
            for j in range(K):
                lg_o = oc.decode([toks[-1]], n_past + j); toks.append(int(np.argmax(lg_o)))
            out, _ = ctx.generate_greedy(n_past, K)
            assert [int(x) for x in out[:K + 1]] == toks, "device greedy loop after a shift: tokens differ"
            same_logits(ctx.last_logits(), lg_o, "device greedy loop, last step")
            n_past += K; greedy_done = True
            continue
        lg_o = oc.decode([t], n_past); same_logits(ctx.decode([t], n_past), lg_o, "step at n_past %d after %d shifts" % (n_past, shifts))
        n_past += 1; s += 1
    assert shifts == 2 and (greedy_done or not (name == "gq4_hd256" and n_ctx == 96))
    if name == "gq2_hd192" and n_ctx == 96:
        oc.kv_seq_rm(n_keep, -1); ctx.kv_seq_rm(n_keep, -1)
        batch = [(31 * i + 5) % 512 for i in range(20)]
        lg_o = oc.decode(batch, n_keep); same_logits(ctx.decode(batch, n_keep), lg_o, "micro-batch after the truncation")
        n_past = n_keep + len(batch)
        for _ in range(4):
            t = int(np.argmax(lg_o))
            lg_o = oc.decode([t], n_past); same_logits(ctx.decode([t], n_past), lg_o, "step after the truncation")
            n_past += 1
    oc.close(); ctx.close(); m.close()


@pytest.mark.parametrize("name", sorted(MODELS))
def test_model_self_extend_vs_oracle(bamd, po, tmp_path, name):
    """Self-Extend (cpp/bridge.cpp:509-522, ga_n 4, ga_w 64) on both sides: a 40-token prompt and 200 greedy steps, every step's logits"""
    n_ctx, ga_n, ga_w = 256, 4, 64
    om, oc, m, ctx = open_pair(bamd, po, tmp_path, name, n_ctx)
    prompt = [(7919 * i + 13) % 512 for i in range(40)]
    lg_o = oc.decode(prompt, 0); same_logits(ctx.decode(prompt, 0), lg_o, "prompt")
    n_past, ga_i, events = len(prompt), 0, 0
    for s in range(200):
        while n_past >= ga_i + ga_w:
            ib, bd = (ga_n * ga_i) // ga_w, (ga_w // ga_n) * (ga_n - 1)
            dd = (ga_w // ga_n) - ib * bd - ga_w
            for c in (oc, ctx):
                c.kv_seq_add(ga_i, n_past, ib * bd)
                c.kv_seq_div(ga_i + ib * bd, ga_i + ib * bd + ga_w, ga_n)
                c.kv_seq_add(ga_i + ib * bd + ga_w, n_past + ib * bd, dd)
            n_past -= bd
            ga_i += ga_w // ga_n
            events += 1
        t = int(np.argmax(lg_o))
        lg_o = oc.decode([t], n_past); same_logits(ctx.decode([t], n_past), lg_o, "step %d after %d windows" % (s, events))
        n_past += 1
    assert events >= 3
    oc.close(); ctx.close(); m.close()
