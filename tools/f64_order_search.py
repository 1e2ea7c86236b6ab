#!/usr/bin/env python3
"""The one documented numerics deviation: the RMSNorm sum of squares is accumulated in double in a fixed TREE
order on the GPU (ActPro::finish, bamd_device.h) and SEQUENTIALLY in the reference (ggml_compute_forward_rms_norm_f32,
cpp/ggml/src/ggml.c:11874-11879); both round the mean to f32 right after.  This tool (CPU only, numpy) restates both orders for
n = 4096 and
  (a) counts, over random activation vectors, how often the f32 mean differs (expected ~1e-8 per reduction);
  (b) CONSTRUCTS an adversarial vector: two elements are tuned until the sum sits a few double-ulps below a rounding boundary of
      the f32 mean, then a tiny last element walks it across one double-ulp at a time; where the two orders cross the boundary
      at different steps the two means differ by one f32 ulp.
    python tools/f64_order_search.py [n_random] [out.npz]
    python tools/f64_order_search.py --near K [seed] [out.npz]
  (c) for ANY length K (construct_near): a vector whose SEQUENTIAL f64 mean sits within NEAR_UNITS = 8 units of an f32 rounding boundary
      (units of f32_rounding_safe: the low 29 mantissa bits D, boundary D = 2^28).  Any other order of the same K terms is within 2 K units of
      the sequential one, i.e. inside the band 2 K + 8 in which the guard refuses the tree: the fallback runs whatever a kernel's tree is.
      tests/golden/gen_f64_guard_kats.py stores such vectors (tests/golden/f64_order_kats.npz) for tests/test_gpu_f64_guard.py.
  (d) the tree of every RMSNorm site for any length (SITE_TREES: sum_tree_blocks = ActPro::finish = ActProQ0::finish_q0, sum_tree_flt = flt_act):
      tests/golden/gen_f64_teeth_kats.py keeps only vectors of (c) on which the site's OWN tree rounds to another f32 mean and another f32 scale than
      the sequential order (tests/golden/f64_teeth_kats.npz): on those a kernel that skipped its fallback gives other output bits.
"""
import sys

import numpy as np

K = 4096


def terms(x):
    x = np.asarray(x, np.float32)
    return (x * x).astype(np.float32).astype(np.float64)           # (ggml_float)(x[i] * x[i]): the product is rounded to f32 first


def sum_seq(t):
    return float(np.cumsum(t, dtype=np.float64)[-1])               # cumsum adds strictly left to right


def sum_tree(t):
    """ActPro<true>::finish for K = 4096, 8 waves: wave w owns blocks w and w + 8; lane l the elements 4l..4l+3 of each, added in
    order; wave_sum_f64 = xor 1, xor 2, half-mirror, mirror inside rows of 16 lanes, then ((r0 + r1) + r2) + r3; the eight wave
    sums are added in order starting from 0."""
    b = t.reshape(16, 64, 4)                                       # [block][lane][element]
    tot = 0.0
    for w in range(8):
        lane = np.zeros(64, np.float64)
        for blk in (w, w + 8):
            for c in range(4):
                lane = lane + b[blk, :, c]
        s = lane
        s = s + s[np.arange(64) ^ 1]
        s = s + s[np.arange(64) ^ 2]
        i = np.arange(64); s = s + s[(i & ~7) | (7 - (i & 7))]
        s = s + s[(i & ~15) | (15 - (i & 15))]
        tot = tot + (((s[15] + s[31]) + s[47]) + s[63])
    return float(tot)


def wave_sum_f64(s):
    """wave_sum_f64 (bamd_device.h) over [64] lane values: s += xor 1, s += xor 2, s += the mirror inside groups of 8 lanes, s += the mirror inside rows
    of 16 lanes (every lane of a row then holds the row's sum), then ((lane 15 + lane 31) + lane 47) + lane 63"""
    i = np.arange(64)
    s = s + s[i ^ 1]
    s = s + s[i ^ 2]
    s = s + s[(i & ~7) | (7 - (i & 7))]
    s = s + s[(i & ~15) | (15 - (i & 15))]
    return float(((s[15] + s[31]) + s[47]) + s[63])


def sum_tree_blocks(t, nwaves=8):
    """ActPro<true>::finish (bamd_device.h) and ActProQ0<true>::finish_q0 (bamd_b32_device.h) for any K that is a multiple of 256: the two hold the same
    statements.  issue(x, nw, K, wave) loads the blocks wave, wave + nwaves, .. (BAMD_ACT_BATCH = 4 of them), the loop behind it the batches that start
    at wave + 4 nwaves, wave + 8 nwaves, ..: wave w owns the 256-blocks i = w (mod nwaves) in increasing order, lane l adds the elements 4l .. 4l+3 of
    each in order; wave_sum_f64; the wave sums are added in order starting from 0 (a wave without a block contributes 0).  sum_tree is this at K = 4096"""
    b = np.asarray(t, np.float64).reshape(-1, 64, 4)                # [block][lane][element]
    tot = 0.0
    for w in range(nwaves):
        lane = np.zeros(64, np.float64)
        for blk in range(w, b.shape[0], nwaves):
            for c in range(4):
                lane = lane + b[blk, :, c]
        tot = tot + wave_sum_f64(lane)
    return float(tot)


def sum_tree_flt(t, nthreads=512):
    """flt_act<true, ..> (bamd_flt_device.h) for any K that is a multiple of 256, 512 threads: thread k4 % 512 adds the float4s k4 = thread, thread + 512,
    .. (elements 4 k4 .. 4 k4 + 3 in order); wave_sum_f64 over the 64 threads of a wave; the eight wave sums are added in order starting from 0.  Threads
    >= K / 4 contribute 0"""
    t = np.asarray(t, np.float64)
    n4 = t.size // 4
    rounds = -(-n4 // nthreads)
    b = np.zeros((rounds * nthreads, 4), np.float64)
    b[:n4] = t.reshape(n4, 4)
    b = b.reshape(rounds, nthreads, 4)                             # [round][thread][element]
    part = np.zeros(nthreads, np.float64)
    for r in range(rounds):
        for c in range(4):
            part = part + b[r, :, c]
    tot = 0.0
    for w in range(nthreads // 64):
        tot = tot + wave_sum_f64(part[w * 64:(w + 1) * 64])
    return float(tot)


# the restated tree of every RMSNorm site (tests/test_gpu_f64_guard.py's table): ActPro::finish and finish_q0 are one function
SITE_TREES = dict(flt=sum_tree_flt, q0=sum_tree_blocks, actpro=sum_tree_blocks)


def scale32(mean, eps):
    """1 / sqrtf(mean + eps) in f32, as the kernels and the oracle's rms_norm compute it (ggml.c:11881)"""
    return np.float32(1.0) / np.sqrt(np.float32(np.float32(mean) + np.float32(eps)), dtype=np.float32)


def mean32(s):
    return np.float32(s / K)


def rounding_safe(v, ulps):
    """bamd_device.h f32_rounding_safe, restated: a double rounds to f32 by its low 29 mantissa bits D (boundary D = 2^28); a relative
    reordering error of (2 n + 8) 2^-53 moves D by at most 2 n + 8, so the f32 cannot depend on the order when |D - 2^28| > 2 n + 8"""
    if v == 0.0:
        return True
    bits = int(np.float64(v).view(np.uint64))
    ex = (bits >> 52) & 0x7ff
    dist = (bits & 0x1fffffff) - 0x10000000
    return 1023 - 126 <= ex <= 1023 + 127 and abs(dist) > ulps


GUARD_ULPS = 2 * K + 8                         # BAMD_F64_GUARD_ULPS(K)


def guarded_mean32(t):
    """what the GPU computes since round 3: the tree sum, unless its f32 mean could depend on the order — then the sequential sum"""
    st = sum_tree(t)
    if rounding_safe(st / K, GUARD_ULPS):
        return mean32(st), False
    return mean32(sum_seq(t)), True


def random_trials(n, rng):
    diff = 0
    for _ in range(n):
        x = (rng.standard_normal(K) * np.exp(rng.standard_normal(K) * 2.0)).astype(np.float32)      # wide dynamic range
        t = terms(x)
        if mean32(sum_seq(t)).view(np.uint32) != mean32(sum_tree(t)).view(np.uint32):
            diff += 1
    return diff


def construct(rng, tries=200):
    for attempt in range(tries):
        x = (rng.standard_normal(K) * np.exp(rng.standard_normal(K) * 2.0)).astype(np.float32)
        x[K - 1] = 0.0
        j1 = int(np.argmin(np.abs(np.abs(x[:K - 1]) - 1.0))); j2 = int(np.argmin(np.abs(np.abs(x[:K - 1]) - 1.0 / 64)))
        if j1 == j2:
            continue
        s0 = sum_seq(terms(x))
        m = mean32(s0)
        mid = (float(m) + float(np.nextafter(m, np.float32(np.inf)))) / 2.0 * K          # the sum at which the f32 mean rounds up
        for j, span in ((j1, 400000), (j2, 400000)):                                    # coarse, then fine: land just below `mid`
            best = None
            base = x[j]
            for d in range(-span, span, max(1, span // 4000)):
                x[j] = np.float32(base).view(np.int32).__add__(d).astype(np.int32).view(np.float32) if False else (np.array([base], np.float32).view(np.int32) + d).view(np.float32)[0]
                s = sum_seq(terms(x))
                gap = mid - s
                if gap > 0 and (best is None or gap < best[0]):
                    best = (gap, x[j])
            if best is None:
                break
            x[j] = best[1]
        if best is None:
            continue
        # walk across with the tiny last element: its square moves the sum by far less than one double-ulp per step of its f32 value
        v = np.float32(2.0 ** -22)
        for step in range(200000):
            x[K - 1] = v
            t = terms(x)
            a, b = mean32(sum_seq(t)), mean32(sum_tree(t))
            if a.view(np.uint32) != b.view(np.uint32):
                return x.copy(), a, b
            if a != m:
                break                                     # both crossed together: try another vector
            v = np.float32(v * np.float32(1.0 + 2.0 ** -9))
    return None


# ---- any length: a vector whose sequential mean is within NEAR_UNITS of a rounding boundary ---------------------------------------------------
NEAR_UNITS = 8


def dist_units(v):
    """|D - 2^28| of doubles (array): the distance from an f32 rounding boundary in the units of f32_rounding_safe"""
    lo = np.asarray(v, np.float64).view(np.uint64) & np.uint64(0x1fffffff)
    return np.abs(lo.astype(np.int64) - (1 << 28))


def mean64(s, K):
    """sum / n in double (ggml.c:11879); for a power of two the kernels multiply by the exact reciprocal: the same double"""
    return np.float64(s) / np.float64(K)


def sum_orders(t):
    """the same terms in the reference's order and in three others: dict name -> double"""
    t = np.asarray(t, np.float64)
    pair = t.copy()
    while pair.size > 1:                                                 # pairwise tree (odd lengths: the last term rides along)
        if pair.size & 1:
            pair = np.concatenate([pair[:-1:2] + pair[1::2], pair[-1:]])
        else:
            pair = pair[0::2] + pair[1::2]
    lanes = np.zeros(64, np.float64)                                     # 64 strided partial sums, then added in order
    for i in range(0, t.size, 64):
        c = t[i:i + 64]
        lanes[:c.size] = lanes[:c.size] + c
    return dict(seq=sum_seq(t), rev=sum_seq(t[::-1]), pairwise=float(pair[0]), lanes64=sum_seq(lanes))


def guard_fires(s, K):
    return not rounding_safe(float(mean64(s, K)), 2 * K + 8)


def construct_near(K, rng, x0=None):
    """x [K] f32 with dist_units(sequential mean) <= NEAR_UNITS.  K - 2 elements are random (the activation-like distribution of random_trials) or
    taken from x0; the last two are searched: the sequential sum is (prefix + t_a) + t_b with the prefix computed once, t_a a coarse term (a typical
    element: its candidates move D over its whole range) and t_b a fine one (below 2^-29 of the sum: steps of a unit or less)."""
    x = (rng.standard_normal(K) * np.exp(rng.standard_normal(K) * 2.0)).astype(np.float32) if x0 is None else np.array(x0, np.float32)
    prefix = sum_seq(terms(x[:K - 2]))
    rms = np.sqrt(prefix)
    best = None                                                          # (score, x): 2 = some order rounds to another f32, 1 = the orders' sums differ, 0 = all equal (an exact sum)
    for attempt in range(64):
        a = (rng.standard_normal(2048) * rms / np.sqrt(K)).astype(np.float32)
        b = (rms * 2.0 ** -(14.5 + 1.5 * rng.random(32768))).astype(np.float32)
        ta, tb = terms(a), terms(b)
        for lo in range(0, a.size, 128):
            m = ((prefix + ta[lo:lo + 128, None]) + tb[None, :]) / np.float64(K)
            for k in np.flatnonzero(dist_units(m).ravel() <= NEAR_UNITS)[:8]:
                y = x.copy()
                y[K - 2], y[K - 1] = a[lo + k // b.size], b[k % b.size]
                o = sum_orders(terms(y))
                assert int(dist_units(mean64(o["seq"], K))) <= NEAR_UNITS
                score = 2 if len({int(np.float32(mean64(v, K)).view(np.uint32)) for v in o.values()}) > 1 else 1 if len(set(o.values())) > 1 else 0
                if best is None or score > best[0]:
                    best = (score, y)
                if score == 2:
                    return y
        if best is not None:
            return best[1]
    return None


def main_near(argv):
    K = int(argv[0]); seed = int(argv[1]) if len(argv) > 1 else 0
    x = construct_near(K, np.random.default_rng(seed))
    assert x is not None, "nothing found"
    o = sum_orders(terms(x))
    for name, s in o.items():
        print("%-9s mean %r (bits %08x), %d units from the boundary, guard fires: %s" % (name, float(np.float32(mean64(s, K))), np.float32(mean64(s, K)).view(np.uint32), int(dist_units(mean64(s, K))), guard_fires(s, K)))
    if len(argv) > 2:
        np.savez_compressed(argv[2], x=x, mean_seq=np.float32(mean64(o["seq"], K)))
        print("wrote", argv[2])


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--near":
        return main_near(sys.argv[2:])
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    rng = np.random.default_rng(17)
    d = random_trials(n, rng)
    print("random vectors: %d of %d have a different f32 mean under the two orders" % (d, n))
    r = construct(rng)
    if r is None:
        print("constructive search: no differing vector found")
        return
    x, a, b = r
    print("constructed: sequential mean %r (bits %08x), tree mean %r (bits %08x)" % (float(a), a.view(np.uint32), float(b), b.view(np.uint32)))
    if len(sys.argv) > 2:
        np.savez_compressed(sys.argv[2], x=x, mean_seq_bits=np.uint32(a.view(np.uint32)), mean_tree_bits=np.uint32(b.view(np.uint32)))
        print("wrote", sys.argv[2])


if __name__ == "__main__":
    main()
