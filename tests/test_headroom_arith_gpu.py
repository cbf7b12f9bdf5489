"""div_cap (csrc/engine.hip), the one division of the headroom kernel, run on the
device on its own through the diagnostic ksg_debug_arith (operation 9: x, a, cap
-> min(floor(x / a), cap)) against Python integers over its whole domain:
0 <= x < 2^63, 1 <= a < 2^63, 0 <= cap < 2^31.  Every comparison is equality.

The operands sit on both sides of each gate: the clip x >= cap * a (and the
128-bit product behind it), and div_small's own gates behind the clip -- 32-bit
operands, x at 2^52, an estimated quotient at 2^20."""
import random

import pytest

from test_arith_gpu import bitlen_draw, differ, run

pytestmark = pytest.mark.gpu

DIV_CAP = 9
CAP_MAX = (1 << 31) - 1
X_MAX = (1 << 63) - 1


def want(x, a, cap):
    return min(x // a, cap)


def check(triples):
    T = sorted({(x, a, c) for x, a, c in triples if 0 <= x <= X_MAX and 1 <= a <= X_MAX and 0 <= c <= CAP_MAX})
    assert T
    xs, as_, cs = [t[0] for t in T], [t[1] for t in T], [t[2] for t in T]
    got = run(DIV_CAP, xs, as_, cs)
    n_bad, first = differ(got, [want(*t) for t in T], xs, as_, cs)
    assert n_bad == 0, (n_bad, len(T), first)
    return len(T)


def test_div_cap_by_bit_length():
    """x, a and cap of every bit length (top bit set, the rest random), all against all caps of a sample."""
    r = random.Random(20261020)
    T = []
    for _ in range(3):
        xs, as_ = [0] + bitlen_draw(r, 1, 63), bitlen_draw(r, 1, 63)
        caps = [0] + bitlen_draw(r, 1, 31)
        for x in xs:
            for a in as_:
                T.append((x, a, r.choice(caps)))
                T.append((x, a, CAP_MAX))
    assert check(T) > 20000


def test_div_cap_quotient_at_the_cap():
    """Quotients of cap - 1, cap, cap + 1 and x = m * a + {-1, 0, 1}: the clip decides by one unit."""
    r = random.Random(7)
    T = []
    for cap in [0, 1, 2, 3, 6, 110, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 30) + 12345, CAP_MAX - 1, CAP_MAX]:
        for a in [1, 2, 3, 7, 1000, (1 << 31) - 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 52) - 1, 1 << 52,
                  (1 << 52) + 1, (1 << 62) + 5, X_MAX] + bitlen_draw(r, 1, 63):
            for m in (cap - 1, cap, cap + 1):
                if m < 0:
                    continue
                for d in (-1, 0, 1, a - 1, a // 2):
                    T.append((m * a + d, a, cap))
    assert check(T) > 3000


def test_div_cap_behind_the_clip():
    """A cap the quotient never reaches, so div_small's gates decide: quotients at 2^20 +- 1, operands at
    2^32 +- 1 and 2^52 +- 1, a = 1, x near 2^63."""
    r = random.Random(11)
    T = []
    edges = [(1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 52) - 1, 1 << 52, (1 << 52) + 1, X_MAX - 1, X_MAX]
    for a in [1, 2, 3, 5, 7, 100, (1 << 12) + 1] + edges + bitlen_draw(r, 1, 63):
        for q in ((1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1, 2, 99, 100, 101, CAP_MAX - 1):
            for d in (-1, 0, 1):
                T.append((q * a + d, a, CAP_MAX))
        for x in edges + [0, 1, a - 1, a, a + 1]:
            for cap in (CAP_MAX, 1 << 20, 6, 0):
                T.append((x, a, cap))
    for x in [X_MAX, X_MAX - 1, (1 << 62), (1 << 62) + 1] + [X_MAX - r.getrandbits(20) for _ in range(50)]:
        for a in [1, 2, 3, (1 << 31), (1 << 32) + 1, (1 << 33) - 1, X_MAX // 3, X_MAX] + bitlen_draw(r, 30, 63):
            for cap in (0, 1, 6, CAP_MAX):
                T.append((x, a, cap))
    assert check(T) > 3000


def test_div_cap_headroom_operands():
    """What the kernel feeds it: free bytes / milli-cpu against a request, clipped to a pod room."""
    r = random.Random(3)
    T = []
    for _ in range(20000):
        a = r.choice([50 * (1 + r.randrange(40)), (64 << 20) * (1 + r.randrange(64)), 1 + r.randrange(8)])
        x = r.choice([r.randrange(0, 64000), r.randrange(0, 512 << 30), r.randrange(0, 8)])
        T.append((x, a, r.choice([0, 1, 6, 110, 250])))
    check(T)
