"""Constructs a softmax row on which the reciprocal of the denominator sits next to a rounding boundary of its f32 — inside the band in which
f32_rounding_safe (bamd_device.h) must send the sum down the reference's sequential order — for tests/test_f64_order.py.

The row has 64 scores s_i (f16-representable, so that an attention test can produce them exactly as dot products k_i . q with q = e_0), head
dimension 64 (the scale 1/8 is an exact scaling), s_0 = 0 the maximum.  61 scores are fixed at random, three are searched: positions 47, 55, 63,
the last elements of the 8-wide groups 5, 6, 7, whose f32 partial sums ((v0+v4)+(v2+v6))+((v1+v5)+(v3+v7)) (ggml.c:2635-2644) are tabulated by
candidate; the sequential double sum of the eight partial sums is then enumerated over all triples.  The exponentials come from the oracle's ggml_v_expf restatement (oracle/, test infrastructure).
usage: python tools/f64_softmax_search.py   -> tests/golden/f64_softmax_kat.npz
       python tools/f64_softmax_search.py --row VALID PADDED KQ_SCALE [seed] [out.npz]

construct_row() is the same search for ANY row: a valid length, a padded length (the tail is masked: score -inf, exponential 0 — a causal micro-batch
or a half-filled last block), holes (masked cells inside the row) and an f32 kq_scale, applied as the reference applies it (f32 product s * kq_scale,
then - max, then the oracle's bo_v_expf).  Its rows have 1 / (sequential sum) within NEAR_UNITS = 8 units of an f32 rounding boundary; any order of
the same n = padded / 8 partial sums is within 2 n units of that, inside the band 2 n + 8 of f32_rounding_safe: the fallback runs whatever the
kernel's tree.  tests/golden/gen_f64_guard_kats.py stores such rows (tests/golden/f64_softmax_kats.npz) for tests/test_gpu_f64_guard.py."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 64
GUARD_ULPS = 2 * (N // 8) + 8                   # BAMD_F64_GUARD_ULPS(n_kv / 8)


def expf_table(po, vals):
    L = po.lib()
    return np.array([L.bo_v_expf(float(v)) for v in vals], np.float32)


def group_sum(v):
    """the reference's 8-wide partial sum, f32"""
    v = v.astype(np.float32)
    a0, a1, a2, a3 = v[0] + v[4], v[1] + v[5], v[2] + v[6], v[3] + v[7]
    return np.float32(np.float32(a0 + a2) + np.float32(a1 + a3))


def dist(rs):
    """|low 29 mantissa bits - 2^28| of doubles: how far the value is from an f32 rounding boundary, in units of the double's ulp"""
    lo = rs.view(np.uint64) & np.uint64(0x1fffffff)
    return np.abs(lo.astype(np.int64) - (1 << 28))


def denominators(e):
    """the row's denominator in the reference's order and in a few others (exps e[64] f32): dict name -> double"""
    c = np.array([group_sum(e[g * 8:g * 8 + 8]) for g in range(N // 8)], np.float64)
    seq = 0.0
    for x in c: seq = seq + x
    rev = 0.0
    for x in c[::-1]: rev = rev + x
    tree = ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]))
    tree2 = ((c[0] + c[4]) + (c[2] + c[6])) + ((c[1] + c[5]) + (c[3] + c[7]))
    return dict(seq=seq, rev=rev, tree=tree, tree2=tree2)


# ---- any row length, masked tail / holes, any scale ----------------------------------------------------------------------------------------
NEAR_UNITS = 8


def row_exps(po, scores, scale):
    """exp(s * kq_scale - max) as bo_soft_max forms it (max = 0 at position 0): f32 product, then the oracle's expf; -inf gives 0"""
    w = (np.asarray(scores, np.float32) * np.float32(scale)).astype(np.float32)
    assert w[0] == 0.0 and np.all(w <= 0.0)
    e = np.zeros(w.size, np.float32)
    ok = np.isfinite(w)
    e[ok] = expf_table(po, w[ok])
    return e


def group_sums(e):
    """the reference's 8-wide f32 partial sums of a whole row (ggml.c:2635-2644), as doubles"""
    v = np.asarray(e, np.float32).reshape(-1, 8)
    a0, a1, a2, a3 = v[:, 0] + v[:, 4], v[:, 1] + v[:, 5], v[:, 2] + v[:, 6], v[:, 3] + v[:, 7]
    return ((a0 + a2).astype(np.float32) + (a1 + a3).astype(np.float32)).astype(np.float32).astype(np.float64)


def row_denominators(e):
    """the denominator of a row of any length in the reference's order and in three others: dict name -> double"""
    c = group_sums(e)
    seq = float(np.cumsum(c)[-1])
    rev = float(np.cumsum(c[::-1])[-1])
    pair = c.copy()
    while pair.size > 1:
        pair = np.concatenate([pair[:-1:2] + pair[1::2], pair[-1:]]) if pair.size & 1 else pair[0::2] + pair[1::2]
    lanes = np.zeros(8, np.float64)                                      # eight strided partial sums, then added in order
    for i in range(0, c.size, 8):
        lanes[:c[i:i + 8].size] = lanes[:c[i:i + 8].size] + c[i:i + 8]
    return dict(seq=seq, rev=rev, pairwise=float(pair[0]), lanes8=float(np.cumsum(lanes)[-1]))


def guard_fires(den, padded):
    """f32_rounding_safe(1 / den, BAMD_F64_GUARD_ULPS(n_kv / 8)) restated: True = the kernel must take the sequential order"""
    return int(dist(np.array([1.0 / den]))[0]) <= 2 * (padded // 8) + 8


def _f16_between(lo, hi):
    """every negative f16 score with lo <= |s| <= hi, as f32"""
    h = np.arange(1, 0x7c00, dtype=np.uint16).view(np.float16).astype(np.float32)
    return -h[(h >= lo) & (h <= hi)]


def construct_row(po, rng, valid, padded, scale, holes=()):
    """scores [padded] f32 (f16-representable, s_0 = 0 the maximum, -inf at the holes and from `valid` on) with dist(1 / sequential sum) <= NEAR_UNITS.
    All but three scores are random; the last elements of the last three valid 8-groups are searched.  The first of these groups lies far below
    the rest of the row (its partial sum moves the denominator in steps below a unit), the other two are ordinary (coarse steps)."""
    assert valid % 8 == 0 and padded % 8 == 0 and 32 <= valid <= padded
    u = np.float32(0.125) / np.float32(scale)                            # the existing row's ranges are those of scale = 1/8
    s = -((rng.random(padded) * 60 + 1) * u).astype(np.float16).astype(np.float32)
    s[0] = 0.0
    G = valid // 8
    gx, gy, gz = G - 3, G - 2, G - 1
    s[gx * 8:gx * 8 + 8] = -((rng.random(8) * 100 + 100) * u).astype(np.float16).astype(np.float32)
    if G >= 6:                                                           # group 1 far below everything (exp 1e-18 .. 1e-13): its partial sum falls off the end of the running double, so the sum is inexact and the order of the additions shows in its last bits
        s[8:16] = -((rng.random(8) * 80 + 240) * u).astype(np.float16).astype(np.float32)
    s[valid:] = -np.inf
    holes = np.asarray(holes, np.int64)
    assert holes.size == 0 or (holes.min() >= 16 and holes.max() < gx * 8)
    s[holes] = -np.inf
    e_f = row_exps(po, s, scale)
    c = group_sums(e_f)
    base = float(np.cumsum(c[:gx])[-1])
    candx, cand = _f16_between(64 * u, 256 * u), _f16_between(1 * u, 64 * u)
    e_cx = expf_table(po, (candx * np.float32(scale)).astype(np.float32)); e_c = expf_table(po, (cand * np.float32(scale)).astype(np.float32))
    def c_of(g, ec):                                                      # the group's partial sum by candidate for its element 7
        v = e_f[g * 8:g * 8 + 8]
        return (((v[0] + v[4]) + (v[2] + v[6])).astype(np.float32) + (np.float32(v[1] + v[5]) + (v[3] + ec)).astype(np.float32)).astype(np.float32).astype(np.float64)
    cx, cy, cz = c_of(gx, e_cx), c_of(gy, e_c), c_of(gz, e_c)
    T1 = base + cx
    best = None                                                          # (score, scores): 2 = some order rounds to another f32, 1 = the orders' sums differ
    for zi in rng.permutation(cand.size)[:48]:
        for lo in range(0, candx.size, 512):
            rs = 1.0 / ((T1[lo:lo + 512, None] + cy[None, :]) + cz[zi])   # (the masked groups behind add 0.0: no change)
            for k in np.flatnonzero(dist(rs).ravel() <= NEAR_UNITS)[:8]:
                r = s.copy()
                r[gx * 8 + 7], r[gy * 8 + 7], r[gz * 8 + 7] = candx[lo + k // cand.size], cand[k % cand.size], cand[zi]
                den = row_denominators(row_exps(po, r, scale))
                assert int(dist(np.array([1.0 / den["seq"]]))[0]) <= NEAR_UNITS
                score = 2 if len({int(np.float32(1.0 / t).view(np.uint32)) for t in den.values()}) > 1 else 1 if len(set(den.values())) > 1 else 0
                if best is None or score > best[0]:
                    best = (score, r)
                if score == 2:
                    return r
        if best is not None and best[0] >= 1:
            return best[1]
    return None if best is None else best[1]


def main_row(argv):
    from oracle import pyoracle as po
    valid, padded, scale = int(argv[0]), int(argv[1]), np.float32(float(argv[2]))
    s = construct_row(po, np.random.default_rng(int(argv[3]) if len(argv) > 3 else 0), valid, padded, scale)
    assert s is not None, "nothing found"
    den = row_denominators(row_exps(po, s, scale))
    for name, t in den.items():
        print("%-9s 1 / sum %r (bits %08x), %d units from the boundary, guard fires: %s" % (name, float(np.float32(1.0 / t)), np.float32(1.0 / t).view(np.uint32), int(dist(np.array([1.0 / t]))[0]), guard_fires(t, padded)))
    if len(argv) > 4:
        np.savez_compressed(argv[4], scores=s, scale=scale, inv_seq=np.float32(1.0 / den["seq"]))
        print("wrote", argv[4])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--row":
        return main_row(sys.argv[2:])
    from oracle import pyoracle as po
    rng = np.random.default_rng(20260927)
    # candidate scores: every f16 in [-64, -1]
    h = np.arange(0x3c00, 0x5401, dtype=np.uint16)                      # 1.0 .. 64.0
    cand = -h.view(np.float16).astype(np.float32)
    e_c = expf_table(po, cand * np.float32(0.125))                      # exp(s / 8 - 0)
    fixed = -(rng.random(N) * 60 + 1).astype(np.float16).astype(np.float32)
    fixed[0] = 0.0
    # groups 1 and 2 far below the rest (exp ~ 1e-18 .. 1e-13): their partial sums fall off the end of the running double, so the ORDER of the
    # eight additions shows in its last bits — the search keeps a row on which the orders round to different f32 reciprocals
    fixed[8:24] = -(rng.random(16) * 80 + 240).astype(np.float16).astype(np.float32)
    fixed[40:48] = -(rng.random(8) * 100 + 100).astype(np.float16).astype(np.float32)     # group 5 too: its searched element moves the denominator in fine steps
    e_f = expf_table(po, fixed * np.float32(0.125))
    # searched positions 47, 55, 63 = the last element of groups 5, 6, 7: the sequential denominator is ((base + c5(x)) + c6(y)) + c7(z) in double
    base = 0.0
    for g in range(5): base = base + float(group_sum(e_f[g * 8:g * 8 + 8]))
    def c_of(g):                                                          # the group's partial sum by candidate for its element 7
        v = e_f[g * 8:g * 8 + 8]
        return (((v[0] + v[4]) + (v[2] + v[6])).astype(np.float32) + (np.float32(v[1] + v[5]) + (v[3] + e_c)).astype(np.float32)).astype(np.float32).astype(np.float64)
    hx = np.arange(0x5400, 0x5c01, dtype=np.uint16)                      # group 5's candidates: every f16 in [-256, -64]
    candx = -hx.view(np.float16).astype(np.float32)
    e_cx = expf_table(po, candx * np.float32(0.125))
    v5 = e_f[40:48]
    c5 = (((v5[0] + v5[4]) + (v5[2] + v5[6])).astype(np.float32) + (np.float32(v5[1] + v5[5]) + (v5[3] + e_cx)).astype(np.float32)).astype(np.float32).astype(np.float64)
    c6, c7 = c_of(6), c_of(7)
    T1 = base + c5
    best = None
    for zi in rng.permutation(cand.size)[:512]:
        for lo in range(0, candx.size, 512):
            rs = 1.0 / ((T1[lo:lo + 512, None] + c6[None, :]) + c7[zi])
            d = dist(rs)
            k = int(np.argmin(d))
            if d.flat[k] <= 3:
                xi, yi = lo + k // cand.size, k % cand.size
                s = fixed.copy(); s[47] = candx[xi]; s[55] = cand[yi]; s[63] = cand[zi]
                e = expf_table(po, s * np.float32(0.125))
                den = denominators(e)
                ds = {n: int(dist(np.array([1.0 / t]))[0]) for n, t in den.items()}
                f32s = {n: np.float32(1.0 / t) for n, t in den.items()}
                nd = len({int(x.view(np.uint32)) for x in f32s.values()})
                print("hit", candx[xi], cand[yi], cand[zi], ds, {n: hex(int(x.view(np.uint32))) for n, x in f32s.items()}, flush=True)
                if max(ds.values()) <= GUARD_ULPS - 8 and (best is None or nd > best[1]):
                    best = (s, nd, den)
        if best is not None and best[1] > 1:
            break
    assert best is not None, "nothing found"
    s, nd, den = best
    out = os.path.join(ROOT, "tests", "golden", "f64_softmax_kat.npz")
    np.savez(out, scores=s, inv_seq=np.float32(1.0 / den["seq"]), inv_tree=np.float32(1.0 / den["tree"]), distinct=np.int32(nd))
    print("saved", out, "distinct f32 reciprocals over the orders:", nd)


if __name__ == "__main__":
    main()
