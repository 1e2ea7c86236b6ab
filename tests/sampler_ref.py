"""Sampler prefilter: a numpy restatement of what booster_amd/csrc/bamd_sampler.hip has to compute, and the seeded cases of its tests
(tests/test_sampler_ref.py on the CPU, tests/test_gpu_sampler.py on the device).

The rule restated is the reference's sample_janus_token (cpp/janus.cpp:235-324) in the form the kernel file's header gives it:
    penalties, per distinct token:  logit = (float) ((double) logit * pre) when pre != 0 (the EOS boost, :235), then `count` times either
        logit = logit * f in float (kind 0, :264) or logit = (float) ((double) logit * d) (kind 1, :255); then, in a Russian context, every token of an
        incompatible class is multiplied by 0.5 (:270-283);
    shortlist: top = the largest logit; when it is positive, every id with !(logit / top < cutoff_of[top]) in float division (:319-323 on the sorted array:
        the quotient is monotone in the logit then, so the cut of the sorted array is this set).  A NaN logit passes that test.
The restatement is held to the genuine sampler's fixtures and to the library's full-sort path in tests/test_sampler_ref.py; nothing here reads the kernel.

numpy's float32 scalars and arrays multiply and divide in IEEE single precision, float64 in double, and astype / np.float32() round to nearest even: each
line below is one rounding, as in the C expression it restates."""
import functools

import numpy as np

F32, F64, U32 = np.float32, np.float64, np.uint32
PEN_DTYPE = np.dtype({"names": ["id", "count", "kind", "f", "d", "pre"], "formats": ["<i4", "<i4", "<i4", "<f4", "<f8", "<f8"],
                      "offsets": [0, 4, 8, 12, 16, 24], "itemsize": 32})            # bamd_logit_penalty
CAP = 1024                                      # BAMD_SHORTLIST_CAP
PEN_CAP = 512                                   # BAMD_PENALTY_CAP
VS = (300, 1024, 1025, 4100, 128256)
CUT_HI, CUT_LO, CUT_MID = F32(0.99), F32(0.90), F32(0.96)
NAN_QUIET, NAN_NEG, NAN_SIGNALLING = 0x7FC00000, 0xFFC00000, 0x7FA00000
FLT_MAX = np.finfo(np.float32).max
COLLECTING = "ABCDH"                            # classes whose cases are meant to collect more than the top itself


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def apply_penalties(logits, pen, halve_class, halve):
    """the logits after the penalty entries (PEN_DTYPE records, distinct ids) and, when halve, the x0.5 pass over halve_class != 0: a new f32 array"""
    out = np.array(logits, np.float32, copy=True)
    with np.errstate(all="ignore"):
        for e in np.asarray(pen, PEN_DTYPE).reshape(-1):
            l = out[e["id"]]
            if e["pre"] != 0.0:
                l = F32(F64(l) * F64(e["pre"]))
            for _ in range(int(e["count"])):
                l = F32(l * F32(e["f"])) if e["kind"] == 0 else F32(F64(l) * F64(e["d"]))
            out[e["id"]] = l
        if halve:
            m = np.asarray(halve_class) != 0
            out[m] = out[m] * F32(0.5)
    return out


def shortlist(logits, cutoff_of):
    """what the head and the candidate set have to be: dict of nan, top_id, top_logit, cutoff, ntop, count and ids (sorted).  top_any_of is set only where
    the rule leaves the top's id open — a top of zero held as -0.0 and +0.0, equal under the reference's comparison — and then lists the ids that may be
    reported.  With nothing but NaN there is no top: top_id -1, top_logit and cutoff None (unspecified)."""
    l = np.asarray(logits, np.float32)
    isnan = np.isnan(l)
    none = np.zeros(0, np.int64)
    if isnan.all():
        return dict(nan=1, top_id=-1, top_logit=None, cutoff=None, ntop=0, count=0, ids=none, top_any_of=None)
    top = l[~isnan].max()
    equal = np.nonzero(l == top)[0]                                      # NaN compares unequal
    top_id = int(equal[0])
    cutoff = F32(np.asarray(cutoff_of, np.float32)[top_id])
    e = dict(nan=int(isnan.any()), top_id=top_id, top_logit=l[top_id], cutoff=cutoff, ntop=0, count=0, ids=none, top_any_of=None)
    if top > 0:
        with np.errstate(all="ignore"):
            ids = np.nonzero(~(l / F32(top) < cutoff))[0]
        e.update(ntop=int(equal.size), count=int(ids.size), ids=ids)
    elif top == 0 and np.unique(np.signbit(l[equal])).size == 2:
        e.update(top_any_of=equal, top_logit=F32(0.0), cutoff=None)
    return e


# ---- what subtly wrong arithmetic would compute (the teeth of the cases) ---------------------------------------------------------------------------
def member_exact(l, top, cutoff):
    with np.errstate(all="ignore"):
        return ~(np.asarray(l, np.float32) / F32(top) < F32(cutoff))


def member_reciprocal(l, top, cutoff):
    """membership were the quotient a multiplication by the rounded reciprocal"""
    with np.errstate(all="ignore"):
        return ~(np.asarray(l, np.float32) * (F32(1.0) / F32(top)) < F32(cutoff))


def member_double(l, top, cutoff):
    """membership were quotient and comparison done in double"""
    with np.errstate(all="ignore"):
        return ~(np.asarray(l, np.float32).astype(np.float64) / F64(F32(top)) < F64(F32(cutoff)))


def ratio_discriminates(l, top, cutoff):
    """where the exact f32 quotient decides differently from BOTH alternatives"""
    x = member_exact(l, top, cutoff)
    return (x != member_reciprocal(l, top, cutoff)) & (x != member_double(l, top, cutoff))


def mul_double(l, d):
    return (np.asarray(l, np.float32).astype(np.float64) * F64(d)).astype(np.float32)


def mul_double_as_float(l, d):
    """the float x double product were the double factor rounded to float first"""
    return np.asarray(l, np.float32) * F32(d)


def mul_sequence(l, f, count):
    x = np.asarray(l, np.float32)
    for _ in range(int(count)):
        x = x * F32(f)
    return x


def mul_power(l, f, count):
    """`count` float multiplications folded into one: by the factor's power rounded to float, and by its power in double"""
    x = np.asarray(l, np.float32)
    return x * F32(F64(F32(f)) ** int(count)), (x.astype(np.float64) * F64(F32(f)) ** int(count)).astype(np.float32)


def ulp_step(x, k):
    """the f32 value k units in the last place away from the positive finite f32 x"""
    return (np.asarray(x, np.float32).view(np.uint32).astype(np.int64) + k).astype(np.uint32).view(np.float32)


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------
class Case:
    """one call of the prefilter: logits() = the shared base of its vocabulary size with a few planted values, a penalty list, the halve switch, the two
    tables.  meta carries what the case's class promises (checked in tests/test_sampler_ref.py)."""

    def __init__(self, cls, name, V, base, ids=(), bits=(), pen=None, halve=0, halve_class=None, cutoff_of=None, **meta):
        self.cls, self.name, self.V, self.base = cls, name, V, base
        self.ids = np.asarray(ids, np.int64).reshape(-1); self.bits = np.asarray(bits, np.uint32).reshape(-1)
        assert self.ids.size == self.bits.size and np.unique(self.ids).size == self.ids.size, name
        self.pen = np.zeros(0, PEN_DTYPE) if pen is None else pen
        self.halve, self.halve_class, self.cutoff_of, self.meta = halve, halve_class, cutoff_of, meta

    def logits(self):
        x = self.base.copy()
        x.view(np.uint32)[self.ids] = self.bits
        return x

    def expect(self):
        """(logits after the penalties, shortlist() of them), read-only; not kept: a vocabulary size has thousands of cases"""
        after = apply_penalties(self.logits(), self.pen, self.halve_class, self.halve)
        after.setflags(write=False)
        return after, shortlist(after, self.cutoff_of)

    def __repr__(self):
        return "%s/V=%d/%s" % (self.cls, self.V, self.name)


def _bits(vals):
    return np.asarray(vals, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def tables(V):
    """halve_class (about 30 % of the ids) and cutoff_of (0.99 / 0.90 per id at random) of a vocabulary size, and its base logits N(2, 1)"""
    rng = np.random.default_rng(500000 + V)
    cls = (rng.random(V) < 0.30).astype(np.uint8)
    cut = np.where(rng.random(V) < 0.5, CUT_HI, CUT_LO).astype(np.float32)
    base = rng.normal(2.0, 1.0, V).astype(np.float32)
    for a in (cls, cut, base):
        a.setflags(write=False)
    return cls, cut, base


def top_positions(V):
    """id 0, id V - 1 and both sides of every multiple of 64 inside V (the multiples of 1024 are among them)"""
    pos = {0, V - 1}
    for b in range(64, V, 64):
        pos.update((b - 1, b))
    return sorted(pos)


def _inner_ids(rng, V, n, exclude=()):
    """n distinct ids away from the block and wave edges (id % 64 in 2..61, not 0 or V - 1) and outside `exclude`"""
    ok = np.ones(V, bool); ok[list(exclude)] = False
    r = np.arange(V) % 64
    ok &= (r >= 2) & (r <= 61); ok[0] = ok[V - 1] = False
    return rng.choice(np.nonzero(ok)[0], n, replace=False)


def _with_cut(cut, top_id, c):
    out = cut.copy(); out[top_id] = c; out.setflags(write=False)
    return out


def find_ratio_boundary(rng, cutoff):
    """(top, l): top in [8, 40) and l within 3 ulp of f32(cutoff * top) such that ratio_discriminates(l, top, cutoff) — found by search"""
    c = F32(cutoff)
    for _ in range(1000):
        tops = rng.uniform(8.0, 40.0, 4096).astype(np.float32)
        base = c * tops
        for k in (0, 1, -1, 2, -2, 3, -3):
            l = ulp_step(base, k)
            hit = np.nonzero(ratio_discriminates(l, tops, c))[0]
            if hit.size:
                return tops[hit[0]], l[hit[0]]
    raise AssertionError("no discriminating ratio found")


def _find_logit(rng, ok):
    """a logit drawn from N(2, 1), away from zero, for which ok(array) holds — found by search"""
    for _ in range(1000):
        l = rng.normal(2.0, 1.0, 256).astype(np.float32)
        l = l[np.abs(l) > 0.25]
        hit = np.nonzero(ok(l))[0]
        if hit.size:
            return l[hit[0]]
    raise AssertionError("no discriminating logit found")


def janus_pre(n_generated, n_max):
    """the EOS factor of janus.cpp:235: 1.0 + log(1.0 + float(pos - promptLen) / float(max)) * 0.05"""
    import math
    return 1.0 + math.log(1.0 + float(F32(n_generated) / F32(n_max))) * 0.05


def penalty_list(V, n_pen, rng, reserved=(), lead=()):
    """n_pen entries at distinct ids outside `reserved`, after the given leading (id, logit) pairs: kinds 0 and 1 alternate, count = 1 + i % 5, entry 4 also carries
    a `pre`; the factors are what the bridge derives from a scale table in [0.8, 1).  Returns (pen, ids, logit bits): each entry's logit is searched so that,
    wherever the entry can tell, wrong arithmetic shows: float x double differs from float x float(double), `count` sequential float products differ from one
    product by the power, the pre applied first differs from the pre applied last (tests/test_sampler_ref.py counts them again)."""
    pen = np.zeros(n_pen, PEN_DTYPE)
    lead = list(lead)[:n_pen]
    taken = set(int(i) for i in reserved) | set(int(i) for i, _ in lead)
    perm = rng.permutation(V)
    free = perm[~np.isin(perm, sorted(taken))][:n_pen - len(lead)].astype(np.int64)
    ids = np.concatenate([np.array([i for i, _ in lead], np.int64), free])
    vals = np.zeros(n_pen, np.float32)
    for i in range(n_pen):
        kind = i % 2 if n_pen >= 8 else 0
        count = 1 + i % 5
        while True:                                   # (about one scale in five gives a d that is a float itself: nothing to tell apart there, draw again)
            scale = F32(rng.uniform(0.8, 1.0))
            d = 1.0 - (1.0 - float(scale)) * 0.20
            if kind == 0 or float(F32(d)) != d:
                break
        pre = janus_pre(17, 100) if (i == 4 and n_pen >= 8) else 0.0
        pen[i] = (ids[i], count, kind, scale, d, pre)
        if i < len(lead):
            vals[i] = lead[i][1]
        elif pre != 0.0:
            def pre_tells(l):                         # the double product from the float one, and the pre before the counts from the pre after them
                first = mul_sequence(mul_double(l, pre), scale, count).view(U32); last = mul_double(mul_sequence(l, scale, count), pre).view(U32)
                return (mul_double(l, pre).view(U32) != mul_double_as_float(l, pre).view(U32)) & (first != last)
            vals[i] = _find_logit(rng, pre_tells)
        elif kind == 1:
            vals[i] = _find_logit(rng, lambda l: mul_double(l, d).view(U32) != mul_double_as_float(l, d).view(U32))
        elif count >= 2:
            def folded(l):
                s = mul_sequence(l, scale, count).view(U32); p32, p64 = mul_power(l, scale, count)
                return (s != p32.view(U32)) & (s != p64.view(U32))
            vals[i] = _find_logit(rng, folded)
        else:
            vals[i] = F32(rng.normal(2.0, 1.0))
    return pen, ids, _bits(vals)


def _plain(V, near, cls, cut, base, top_id, name, klass="A"):
    """N(2, 1) with a unique top of 12.0 at top_id and six values at 0.995 .. 0.80 of it (at `near`): a handful of candidates under either cut-off"""
    vals = (F32(12.0) * np.array([0.995, 0.97, 0.95, 0.91, 0.89, 0.80], np.float32)).astype(np.float32)
    return Case(klass, name, V, base, np.concatenate([[top_id], near]), np.concatenate([_bits([12.0]), _bits(vals)]), halve_class=cls, cutoff_of=cut)


@functools.lru_cache(maxsize=None)
def cases(V):
    """every case of a vocabulary size, in a fixed order (seeded by V): the list tests/test_gpu_sampler.py runs and tests/test_sampler_ref.py audits"""
    cls, cut, base = tables(V)
    rng = np.random.default_rng(900000 + V)
    out = []
    # A. plain: the top at every position where a block, a wave or the array ends
    near = _inner_ids(rng, V, 6)                                              # no top position is among them: those are edge ids
    for p in top_positions(V):
        out.append(_plain(V, near, cls, cut, base, p, "top@%d" % p))
    # B. ratio-test boundary: 16 copies of a logit whose membership only the exact f32 quotient gets right, and its neighbours within 3 ulp of cutoff * top
    for c in (CUT_HI, CUT_LO, CUT_MID):
        for rep in range(2):
            top, l = find_ratio_boundary(rng, c)
            ids = _inner_ids(rng, V, 1 + 16 + 14)
            around = np.repeat(ulp_step(np.full(7, c * top, np.float32), np.arange(-3, 4)), 2)
            bits = np.concatenate([_bits([top]), np.full(16, _bits([l])[0], np.uint32), _bits(around)])
            out.append(Case("B", "cut%.2f#%d" % (c, rep), V, base, ids, bits, halve_class=cls, cutoff_of=_with_cut(cut, ids[0], c), planted=ids[1:17]))
    # C. the 1024-entry cap: exactly n candidates, the top among them
    if V >= 4100:
        for n in (CAP - 1, CAP, CAP + 1, 3000):
            ids = rng.choice(V, n, replace=False)
            vals = (F32(30.0) * (1.0 - rng.uniform(0.0, 0.004, n))).astype(np.float32)
            vals[0] = F32(30.01)
            out.append(Case("C", "n%d" % n, V, base, ids, _bits(vals), halve_class=cls, cutoff_of=cut, n=n))
    # D. ties at the top: two and three equal top logits, the last one in the array's last block; one logit an ulp below them
    for ids in ((5, V - 1), (5, V // 2, V - 1)):
        below = _inner_ids(rng, V, 2, exclude=ids)
        out.append(Case("D", "ties%d" % len(ids), V, base, np.concatenate([ids, below]), _bits([12.0] * len(ids) + [ulp_step(F32(12.0), -1), 11.0]), halve_class=cls, cutoff_of=cut,
                        ntop=len(ids)))
    # E. top <= 0
    neg = (-np.abs(base) - F32(1.0)).astype(np.float32); neg.setflags(write=False)
    zi = _inner_ids(rng, V, 3)
    out.append(Case("E", "negative", V, neg, halve_class=cls, cutoff_of=cut))
    out.append(Case("E", "top+0", V, neg, zi[:1], [0x00000000], halve_class=cls, cutoff_of=cut))
    zs = np.sort(zi)
    out.append(Case("E", "-0<+0", V, neg, zs, [0x80000000, 0x00000000, 0x80000000], halve_class=cls, cutoff_of=cut))          # -0.0 at the lowest id
    out.append(Case("E", "+0<-0", V, neg, zs, [0x00000000, 0x80000000, 0x00000000], halve_class=cls, cutoff_of=cut))
    # F. NaN: one at each edge position in each bit pattern, several at once, nothing else
    top_id = int(_inner_ids(rng, V, 1, exclude=near)[0])
    plain = _plain(V, near, cls, cut, base, top_id, "unused")
    for p in [p for p in (0, 63, 64, 1023, 1024, V - 1) if p < V]:
        for nm, pat in (("quiet", NAN_QUIET), ("negquiet", NAN_NEG), ("signalling", NAN_SIGNALLING)):
            keep = plain.ids != p
            out.append(Case("F", "%s@%d" % (nm, p), V, base, np.concatenate([plain.ids[keep], [p]]), np.concatenate([plain.bits[keep], [pat]]),
                            halve_class=cls, cutoff_of=cut, n_nan=1))
    several = _inner_ids(rng, V, 5, exclude=plain.ids)
    out.append(Case("F", "several", V, base, np.concatenate([plain.ids, several]),
                    np.concatenate([plain.bits, [NAN_QUIET, NAN_NEG, NAN_SIGNALLING, 0x7FFFFFFF, 0xFF800001]]), halve_class=cls, cutoff_of=cut, n_nan=5))
    allnan = np.full(V, NAN_QUIET, np.uint32).view(np.float32); allnan.setflags(write=False)
    out.append(Case("F", "all", V, allnan, [0, V - 1], [NAN_SIGNALLING, NAN_NEG], halve_class=cls, cutoff_of=cut, n_nan=V))
    # G. infinities, subnormals, +-FLT_MAX
    gi = _inner_ids(rng, V, 8)
    out.append(Case("G", "inf", V, base, gi, _bits([np.inf, np.inf, -np.inf, -np.inf, FLT_MAX, -FLT_MAX, 1e30, 0.0]), halve_class=cls, cutoff_of=cut))
    si = _inner_ids(rng, V, 40)
    sub_top = 0x00700000
    sub = np.concatenate([[sub_top], np.rint(sub_top * rng.uniform(0.5, 1.0, 25)).astype(np.uint32),
                          (np.rint(sub_top * np.repeat([0.99, 0.90], 7)).astype(np.int64) + np.tile(np.arange(-3, 4), 2)).astype(np.uint32)]).astype(np.uint32)
    sub[1:][sub[1:] >= sub_top] = sub_top - 1
    out.append(Case("G", "subnormal", V, neg, si, sub, halve_class=cls, cutoff_of=cut))
    out.append(Case("G", "fltmax", V, base, gi, _bits([FLT_MAX, -FLT_MAX, -FLT_MAX, FLT_MAX * F32(0.995), FLT_MAX * F32(0.95), FLT_MAX * F32(0.5), 1e38, -1e38]),
                    halve_class=cls, cutoff_of=cut))
    # H. penalties: the list's block edges and its cap, both kinds, counts 1..5, a pre, ids 0 and V - 1, a dethroned top, a raised negative logit, the x0.5 pass
    top_h = int(np.nonzero((cls != 0) & (np.arange(V) % 64 >= 2) & (np.arange(V) % 64 <= 61))[0][7])           # unpenalised, in the halved class
    was_top = int(_inner_ids(rng, V, 1, exclude=(top_h,))[0])
    negative = int(_inner_ids(rng, V, 1, exclude=(top_h, was_top))[0])
    for n_pen, halve in [(n, 0) for n in (0, 1, 255, 256, 257, PEN_CAP) if n <= V - 8] + [(256, 1), (0, 1)]:
        lead = [(V - 1, F32(3.5)), (0, F32(2.5)), (negative, F32(-3.0)), (was_top, F32(25.0))]
        pen, ids, bits = penalty_list(V, n_pen, rng, reserved=(top_h,), lead=lead)
        if n_pen >= 4:
            pen[3]["kind"], pen[3]["count"], pen[3]["f"] = 0, 2, F32(0.5)                                       # 25.0 -> 6.25: no longer the top
        near_h = _inner_ids(rng, V, 4, exclude=[top_h] + [int(i) for i in ids] + (list(np.nonzero(cls)[0]) if halve else []))    # outside the halved class
        nb = _bits(F32(10.0 if halve else 20.0) * np.array([0.995, 0.95, 0.91, 0.89], np.float32))              # candidates of the top after the pass
        out.append(Case("H", "pen%d%s" % (n_pen, "+halve" if halve else ""), V, base, np.concatenate([[top_h], near_h, ids]),
                        np.concatenate([_bits([20.0]), nb, bits]), pen=pen, halve=halve, halve_class=cls, cutoff_of=cut, top=top_h,
                        was_top=was_top if n_pen >= 4 else None, negative=negative if n_pen >= 3 else None))
    # the x0.5 pass changes who is the top: 15.0 in the halved class (7.5 after it) beside 10.0 outside it
    rival, *around = _inner_ids(rng, V, 4, exclude=[top_h] + list(np.nonzero(cls)[0]))
    out.append(Case("H", "halve-dethrones", V, base, [top_h, rival] + around, _bits([15.0, 10.0, 9.95, 9.2, 7.6]), halve=1, halve_class=cls, cutoff_of=cut,
                    top=int(rival), was_top=top_h, negative=None))
    return out


def pick(V, klass, name=None):
    return [c for c in cases(V) if c.cls == klass and (name is None or c.name == name)]


def refused_penalties(V):
    """PEN_CAP + 1 entries (ids may repeat where V is small: the call is refused before it reads them)"""
    pen = np.zeros(PEN_CAP + 1, PEN_DTYPE)
    pen["id"] = np.arange(PEN_CAP + 1) % V; pen["count"] = 1; pen["f"] = F32(0.5); pen["d"] = 0.5
    return pen
