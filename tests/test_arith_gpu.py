"""The engine's arithmetic fast paths, run on the device on their own
(ksg_debug_arith -> k_selftest_arith, csrc/engine.hip: the very __device__
functions the kernels call) against exact host references: Python integers for
the integer quotients, Python floats (IEEE binary64, one rounding per operation,
no contraction: what Go and the oracle compute) for the fractions and the
BalancedAllocation scores, the oracle's go_log for go_log.  Every comparison is
equality.  The operands sit on both sides of every domain gate (2^32, 2^52 and the
quotient 2^20 in div_small, 2^45 in the class path's doubles, 2^20 in norm_div;
least_req_q has none up to a < 2^56, and is run across 2^52, where one stood) and on the quotient boundaries m*a - 1, m*a, m*a + 1, where an
estimate that is one off changes the floor.

tests/test_markstein.py proves the class path's division identity in C on the
CPU; test_wc_frac here runs the device code on the same domain.
tests/test_magnitude_gpu.py drives the same gates end to end."""
import ctypes
import math
import random
import struct

import numpy as np
import pytest

from _oracle import go_log
from ksg import load_library

DIV_SMALL, LEAST_REQ_Q, LEAST_REQ_D, UDIV_SMALL, NORM_DIV, WC_FRAC, BA, GO_LOG, IPA_NORM = range(9)
I64 = ctypes.POINTER(ctypes.c_int64)


def run(op, *cols):
    """One launch: op over the columns (equal-length lists of Python ints in int64)."""
    n = len(cols[0])
    assert n and all(len(c) == n for c in cols)
    a = np.ascontiguousarray(np.array(cols, dtype=np.int64))
    out = np.zeros(n, dtype=np.int64)
    L = load_library()
    L.ksg_debug_arith.argtypes = [ctypes.c_int, I64, ctypes.c_uint32, I64, ctypes.c_uint32]
    rc = L.ksg_debug_arith(op, a.ctypes.data_as(I64), len(cols), out.ctypes.data_as(I64), n)
    assert rc == 0, rc
    return out.tolist()


def bits(f):
    return struct.unpack("<q", struct.pack("<d", f))[0]


def unbits(i):
    return struct.unpack("<d", struct.pack("<q", i))[0]


def differ(got, want, *cols, limit=6):
    """The first few operands whose result differs, and how many do."""
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    return len(bad), [(tuple(c[i] for c in cols), got[i], want[i]) for i in bad[:limit]]


def bitlen_draw(r, lo, hi):
    """One integer of every bit length lo..hi (top bit set)."""
    return [(1 << (b - 1)) | r.getrandbits(b - 1) if b > 1 else 1 for b in range(lo, hi + 1)]


# ------------------------------------------------------------------ div_small
# found by this test: 2^32 / 3 came out 4 low (the f64 reciprocal estimate is good to
# about 2^-28, and only an estimate that is one off was corrected); fixed by sending
# quotients of 2^20 and more to the 64-bit divide
DIV_SMALL_FOUND = [(1 << 32, 3), (1 << 32, 5), (1 << 32, 7), ((1 << 32) + 1, 3)]


def div_small_gate_pairs(r):
    P = list(DIV_SMALL_FOUND)
    small = list(range(1, 130)) + [255, 256, 257, 1000, 4095, 4096, 65535, 65536, 65537]
    for x in ((1 << 32) - 1, 1 << 32, (1 << 32) + 1):
        P += [(x, a) for a in small]
    for a in ((1 << 32) - 1, 1 << 32, (1 << 32) + 1):
        for x in (0, 1, a - 1, a, a + 1, 50 * a - 1, 50 * a, 100 * a - 1, 100 * a, 100 * a + 1, (1 << 32) - 1, 1 << 32,
                  (1 << 52) - 1, 1 << 52):
            P.append((x, a))
    # the 2^52 gate: a of every bit length (any quotient), and a near x / m (the callers' quotients)
    for a in bitlen_draw(r, 1, 56) + [(1 << 52) // m + d for m in range(1, 101) for d in (-1, 0, 1)]:
        for x in ((1 << 52) - a, (1 << 52) - 1, 1 << 52, (1 << 52) + 1, (1 << 56) + 1, 1 << 62):
            if x >= 0:
                P.append((x, a))
    # the quotient gate: estimates of 2^20 and more take the 64-bit divide
    for a in bitlen_draw(r, 1, 32) + [3, 5, 7, 100, (1 << 12) + 1, (1 << 31) - 1, (1 << 32) - 1, (1 << 32) + 1]:
        for Q in ((1 << 20) - 2, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 20) + 2):
            P += [(x, a) for x in (Q * a - 1, Q * a, Q * a + 1, Q * a + a - 1, Q * a + a // 2)]
    return P


def div_small_boundary_pairs(r):
    """x = m*a - 1, m*a, m*a + 1 for a of every bit length 1..56, m in [0, 100]."""
    P = []
    for _ in range(6):
        for a in bitlen_draw(r, 1, 56):
            for m in range(101):
                P += [(x, a) for x in (m * a - 1, m * a, m * a + 1) if x >= 0]
    return P


def div_small_weighted_pairs(r, n):
    """The callers' domain with a weight folded in: x <= 100 * w * a, w up to 2^14."""
    P = []
    while len(P) < n:
        a = (1 << r.randrange(0, 40)) + r.getrandbits(20)
        w = 1 << r.randrange(0, 15)
        m = r.randrange(0, 100 * w + 1)
        x = m * a + r.choice((-1, 0, 0, 1, r.randrange(a)))
        if 0 <= x < 1 << 62:
            P.append((x, a))
    return P


# the documented domain "0 <= x < 2^52, a > 0" away from the callers' quotients
LARGE_Q_NAMED = [((1 << 52) - 1, 3), ((1 << 52) - 1, 5), ((1 << 52) - 1, 7), ((1 << 52) - 1, (1 << 32) + 1),
                 (3 * ((1 << 50) + 12345) + 2, 3), (7 * ((1 << 49) - 1), 7), (5 * (1 << 49) - 1, 5)]


def div_small_large_quotient_pairs(r, n):
    P = list(LARGE_Q_NAMED)
    while len(P) < n:
        a = r.choice((3, 5, 7, (1 << 32) + 1))
        x = r.getrandbits(r.randrange(33, 53))
        q = x // a
        P += [(v, a) for v in (x, q * a, q * a + a - 1) if 0 <= v < 1 << 52]
    return P


def check_div(P):
    xs, as_ = [p[0] for p in P], [p[1] for p in P]
    got = run(DIV_SMALL, xs, as_)
    n, bad = differ(got, [x // a for x, a in P], xs, as_)
    assert n == 0, (n, len(P), bad)


@pytest.mark.gpu
def test_div_small_gates_and_quotient_boundaries():
    r = random.Random(0xD1F5)
    P = div_small_gate_pairs(r) + div_small_boundary_pairs(r) + div_small_weighted_pairs(r, 30000)
    assert len(P) > 100000
    assert sum(1 for x, a in P if x <= 0xFFFFFFFF and a <= 0xFFFFFFFF) > 1000  # each branch is met
    assert sum(1 for x, a in P if x >= 1 << 52) > 1000
    check_div(P)


@pytest.mark.gpu
def test_div_small_large_quotients():
    """div_small's documented domain away from its callers' quotients (<= 100 x a
    weight): 0 <= x < 2^52 with a in {3, 5, 7, 2^32 + 1}."""
    check_div(div_small_large_quotient_pairs(random.Random(0xD1F6), 100000))


# ------------------------------------------------------------------ leastRequestedScore
def least_req_pairs(r, top):
    """(a, q): a of every bit length up to top; a a multiple of 100 with q = k*a/100 and
    its neighbour; q in {0, 1, a-1, a, a+1}."""
    P = []
    for _ in range(4):
        for a in bitlen_draw(r, 1, top):
            P += [(a, q) for q in (0, 1, a - 1, a, a + 1, r.randrange(a + 1), r.randrange(a + 1))]
    for _ in range(11):
        for b in range(1, top - 6):
            a = 100 * ((1 << (b - 1)) | r.getrandbits(b - 1))
            if a.bit_length() > top:
                continue
            for k in range(101):
                P += [(a, k * a // 100), (a, k * a // 100 + 1)]
    return [(a, q) for a, q in P if q >= 0]


def least_want(a, q):
    return 0 if q > a or a <= 0 else (a - q) * 100 // a


@pytest.mark.gpu
def test_least_req_q():
    r = random.Random(0x1EA5)
    P = least_req_pairs(r, 56)
    g = (1 << 52) // 100
    P += [(g, 0), (g + 1, 0), (g, 1), (g + 1, 1), (2 * g, g), (2 * g + 2, g), (2 * g + 2, g + 1), (0, 0), (0, 5)]
    assert len(P) > 80000 and sum(1 for a, q in P if (a - q) * 100 >= 1 << 52) > 1000
    a_, q_ = [p[0] for p in P], [p[1] for p in P]
    n, bad = differ(run(LEAST_REQ_Q, a_, q_), [least_want(a, q) for a, q in P], a_, q_)
    assert n == 0, (n, len(P), bad)


@pytest.mark.gpu
def test_least_req_d():
    """The class path's form: allocatable a < 2^45, NonZeroRequested nz and the pod's
    request p (< 2^44) as doubles, x = (a - nz) * 100 - p * 100, the reciprocal 1.0 / a."""
    r = random.Random(0x1EA6)
    T = []
    lim, plim = (1 << 45) - 1, (1 << 44) - 1
    for a, q in least_req_pairs(r, 45) + [(lim, 0), (lim, 1), (lim, lim), (lim, lim - 1), (lim, plim), (lim, plim + 1)]:
        if a > lim or q > 2 * lim:
            continue
        for p in {0, min(q, plim), min(q, r.randrange(plim + 1))}:
            T.append((a, q - p, p))
    T += [(lim, lim, plim), (lim, lim + (200 << 20), 0), (1, 0, plim), (0, 0, 0), (lim, 0, plim)]
    assert len(T) > 80000
    cols = [[t[k] for t in T] for k in range(3)]
    n, bad = differ(run(LEAST_REQ_D, *cols), [least_want(a, nz + p) for a, nz, p in T], *cols)
    assert n == 0, (n, len(T), bad)


# ------------------------------------------------------------------ normalisers
def norm_pairs(r):
    P = []
    for d in range(1, 4097):
        for m in range(101):
            P += [(x, d) for x in (m * d - 1, m * d) if x >= 0]
    return P


@pytest.mark.gpu
def test_udiv_small():
    """x < 2^27, quotient <= 128: every d in [1, 4096] at every quotient boundary
    m d - 1, m d for m <= 100, and d up to 2^20 (the largest normaliser norm_div hands it)."""
    r = random.Random(0x0D17)
    P = norm_pairs(r)
    for d in [(1 << 20) - 1, (1 << 20) - 2, 1 << 19, (1 << 19) + 1, 1000003 % (1 << 20)] + \
            [r.randrange(4097, 1 << 20) for _ in range(2000)]:
        P += [(x, d) for x in (0, d - 1, d, 100 * d - 1, 100 * d, r.randrange(100 * d + 1))]
    assert all(x < 1 << 27 and x // d <= 128 for x, d in P) and len(P) > 100000
    xs, ds = [p[0] for p in P], [p[1] for p in P]
    n, bad = differ(run(UDIV_SMALL, xs, ds), [x // d for x, d in P], xs, ds)
    assert n == 0, (n, len(P), bad)


@pytest.mark.gpu
def test_norm_div_across_its_switch():
    r = random.Random(0x0D18)
    P = norm_pairs(r)
    for d in ((1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 31) - 1, 1 << 40):
        P += [(x, d) for x in (0, d - 1, d, 100 * d - 1, 100 * d)]
        P += [(m * d + e, d) for m in range(100) for e in (-1, 0, 1) if m * d + e >= 0]
    # PodTopologySpread's 100 * (mx + mn - s), mn > 0, mn <= s <= mx
    for _ in range(20000):
        mx = r.choice((r.randrange(1, 4096), r.randrange(1, 1 << 21), (1 << 20) + r.randrange(-3, 4)))
        mn = r.randrange(1, mx + 1)
        s = r.choice((mn, mx, r.randrange(mn, mx + 1)))
        P.append((100 * (mx + mn - s), mx))
    assert len(P) > 100000
    xs, ds = [p[0] for p in P], [p[1] for p in P]
    n, bad = differ(run(NORM_DIV, xs, ds), [x // d for x, d in P], xs, ds)
    assert n == 0, (n, len(P), bad)


# ------------------------------------------------------------------ the class path's division
@pytest.mark.gpu
def test_wc_frac():
    """RN(a / b) from RN(1 / b) and two FMAs (Markstein), on the device, over the
    domain tests/test_markstein.py proves on the CPU: b < 2^45, a < 2^46."""
    r = random.Random(0x3A27)
    P = []
    for e in range(46):
        b = 1 << e
        P += [(a, bb) for bb in (b - 1, b, b + 1) if 0 < bb < 1 << 45
              for a in (0, 1, bb - 1, bb, bb + 1, 2 * bb - 1, b - 1, b + 1, (1 << 46) - 1, (1 << 45) + 1)]
    for _ in range(44):
        for lb in range(1, 46):
            for la in range(1, 47):
                P.append((r.getrandbits(la), (1 << (lb - 1)) | r.getrandbits(lb - 1)))
    for b in range(1, 300):
        P += [(a, b) for a in range(0, 2 * b + 1)]
    assert len(P) > 100000 and all(0 <= a < 1 << 46 and 0 < b < 1 << 45 for a, b in P)
    a_, b_ = [p[0] for p in P], [p[1] for p in P]
    n, bad = differ(run(WC_FRAC, a_, b_), [bits(float(a) / float(b)) for a, b in P], a_, b_)
    assert n == 0, (n, len(P), bad)


# ------------------------------------------------------------------ BalancedAllocation
def ba_want(pairs):
    """balanced_allocation.go balancedResourceScorer over (requested, allocatable) pairs."""
    fr = []
    for q, a in pairs:
        if a == 0:
            continue
        f = float(q) / float(a)
        fr.append(1.0 if f > 1 else f)
    sd = 0.0
    if len(fr) == 2:
        sd = abs((fr[0] - fr[1]) / 2)
    elif len(fr) > 2:
        total = 0.0
        for f in fr:
            total = total + f
        mean = total / float(len(fr))
        s = 0.0
        for f in fr:
            s = s + (f - mean) * (f - mean)
        sd = math.sqrt(s / float(len(fr)))
    return int((1 - sd) * 100.0)


def near_integer_ba2(r):
    """Two-resource cases whose exact (1 - |f0 - f1| / 2) * 100 is an integer k:
    f1 = p / (50 t), f0 = (p + j t) / (50 t), both scaled by unrelated factors; the
    binary64 value lands on k or a few ulps beside it, where truncation decides."""
    out = []
    for _ in range(60000):
        t, j = r.randrange(1, 400), r.randrange(0, 51)
        p = r.randrange(0, 50 * t - j * t + 1)
        u, v = r.choice((1, 3, 7, 1 << 20, 1000003, (1 << 33) + 9)), r.choice((1, 5, 11, 1 << 27, 999983))
        c = ((p + j * t) * u, 50 * t * u, p * v, 50 * t * v)
        f0, f1 = float(c[0]) / float(c[1]), float(c[2]) / float(c[3])
        val = (1 - abs((f0 - f1) / 2)) * 100.0
        k = round(val)
        if abs(val - k) <= 4 * math.ulp(val) and r.random() < 0.5:
            out.append(c if r.random() < 0.5 else (c[2], c[3], c[0], c[1]))
    return out


def magnitudes(r, n, k):
    """n rows of k (q, a) pairs, a at every magnitude up to 2^56, q around a's."""
    rows = []
    while len(rows) < n:
        row = []
        for _ in range(k):
            a = (1 << r.randrange(0, 56)) + r.getrandbits(r.randrange(1, 40))
            q = r.choice((0, 1, a - 1, a, r.randrange(a + 1), r.randrange(a + 1), r.randrange(a + 1)))
            row += [q, a]
        rows.append(tuple(row))
    return rows


def ba_rows(r, k):
    rows = magnitudes(r, 60000, k)
    for row in magnitudes(r, 8000, k):  # equal fractions: deviation 0, score 100
        q, a = row[0], row[1]
        s = [r.choice((1, 2, 3, 10, 1 << 10)) for _ in range(k)]
        rows.append(tuple(v for m in s for v in (q * m, a * m)))
    for row in magnitudes(r, 8000, k):  # one fraction clamped at 1 (requested above allocatable)
        i = r.randrange(k)
        row = list(row)
        row[2 * i] = row[2 * i + 1] + r.choice((1, 1 << 20, row[2 * i + 1]))
        rows.append(tuple(row))
    for row in magnitudes(r, 4000, k):  # allocatable 0: the resource is skipped
        i = r.randrange(k)
        row = list(row)
        row[2 * i + 1] = 0
        rows.append(tuple(row))
    return [row for row in rows if all(0 <= v < 1 << 62 for v in row)]


def check_ba(rows, k):
    cols = [[row[c] for row in rows] for c in range(2 * k)]
    want = [ba_want([(row[2 * i], row[2 * i + 1]) for i in range(k)]) for row in rows]
    n, bad = differ(run(BA, *cols), want, *cols)
    assert n == 0, (n, len(rows), bad)


@pytest.mark.gpu
def test_ba_two_resources():
    r = random.Random(0xBA02)
    near = near_integer_ba2(r)
    assert len(near) >= 1000, len(near)
    rows = ba_rows(r, 2) + near
    assert len(rows) > 80000
    check_ba(rows, 2)


def near_integer_ba4(r):
    """Four-resource cases whose exact (1 - std) * 100 is an integer: fractions
    m + d, m + d, m - d, m - d in any order with d = j / 100 have mean m and standard
    deviation exactly d; m = p / (100 t), each fraction scaled by an unrelated factor.
    In binary64 the value lands on the integer or a few ulps beside it.  (Three
    fractions have no such cases: with deviations d1 + d2 + d3 = 0 the variance is
    2 (d1^2 + d1 d2 + d2^2) / 3, and d1^2 + d1 d2 + d2^2 = 6 s^2 has no rational solution
    but 0, the norm form never holding the prime 2 to an odd power; a random search
    meets a few-ulp neighbour of an integer about once in 10^13 draws.)"""
    out = []
    for _ in range(40000):
        t, j = r.randrange(1, 300), r.randrange(0, 51)
        p = r.randrange(j * t, 100 * t - j * t + 1)
        row, val = [], []
        for sgn in r.sample((1, 1, -1, -1), 4):
            u = r.choice((1, 3, 7, 1 << 20, 1000003, (1 << 33) + 9))
            row += [(p + sgn * j * t) * u, 100 * t * u]
        v = ba_exact(row)
        if abs(v - round(v)) <= 4 * math.ulp(v):
            out.append(tuple(row))
    return out


def ba_exact(row):
    """(1 - std) * 100 before truncation, as ba_want forms it (more than two fractions)."""
    fr = [min(float(row[2 * i]) / float(row[2 * i + 1]), 1.0) for i in range(len(row) // 2)]
    total = 0.0
    for f in fr:
        total = total + f
    mean = total / float(len(fr))
    s = 0.0
    for f in fr:
        s = s + (f - mean) * (f - mean)
    return (1 - math.sqrt(s / float(len(fr)))) * 100.0


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 4])
def test_ba_many_resources(k):
    """The mean / squared-deviation / sqrt branch over 3 and 4 fractions; over 4, at
    least 1,000 cases within a few ulps of an integer score (near_integer_ba4)."""
    r = random.Random(0xBA00 + k)
    rows = ba_rows(r, k)
    if k == 4:
        near = near_integer_ba4(r)
        assert len(near) >= 1000, len(near)
        rows += near
    for _ in range(20000):  # small-integer ratios: exact means and squares near representable values
        a = r.randrange(1, 200)
        rows.append(tuple(v for _ in range(k) for v in (r.randrange(0, a + 1), a)))
    check_ba(rows, k)


# ------------------------------------------------------------------ go_log, InterPodAffinity
@pytest.mark.gpu
def test_go_log():
    """Every log(size + 2) argument of PodTopologySpread's weights up to cfg4's sizes,
    and the argument-reduction edges: powers of two and sqrt(2)/2 +- 1 ulp, subnormals."""
    X = [float(i) for i in range(2, 70001)]
    for e in range(-1074, 1024, 7):
        p = math.ldexp(1.0, e)
        X += [p, math.nextafter(p, math.inf)] + ([math.nextafter(p, 0.0)] if e > -1074 else [])
    h = math.sqrt(2.0) / 2
    X += [0.5, h, math.nextafter(h, 0.0), math.nextafter(h, 1.0), 0.70710678118654752440, 1.0, 5e-324, 2.5e-320,
          2.2250738585072014e-308, 1.7976931348623157e308, math.inf, 0.0]
    r = random.Random(0x106)
    X += [math.ldexp(r.random() + 0.5, r.randrange(-1070, 1020)) for _ in range(30000)]
    xb = [bits(x) for x in X]
    n, bad = differ(run(GO_LOG, xb), [bits(go_log(x)) for x in X], X)
    assert n == 0, (n, len(X), bad)


@pytest.mark.gpu
def test_ipa_norm():
    """int64(100 * float64(s - mn) / float64(mx - mn)), 0 when mx == mn."""
    r = random.Random(0x19A)
    T = []
    for _ in range(34000):
        diff = r.choice((r.randrange(1, 200), r.getrandbits(r.randrange(1, 41)) + 1, 1 << 40))
        mn = r.choice((0, -diff, r.randrange(-(1 << 40), 1 << 40), -r.getrandbits(30), r.getrandbits(30)))
        mx = mn + diff
        for s in (mn, mx, mn + r.randrange(diff + 1)):
            T.append((s, mn, mx))
    for d in range(1, 400):  # every k * d / 100 boundary of small ranges
        T += [(s, 0, d) for s in range(d + 1)][:120]
    T += [(5, 5, 5), (-7, -7, -7), (0, 0, 0)]
    assert len(T) > 100000
    cols = [[t[k] for t in T] for k in range(3)]

    def want(s, mn, mx):
        d = mx - mn
        return int(100.0 * (float(s - mn) / float(d))) if d > 0 else 0
    n, bad = differ(run(IPA_NORM, *cols), [want(*t) for t in T], *cols)
    assert n == 0, (n, len(T), bad)
