"""Built cells for the SLOPE block's fit (include/d2pc_sectors.h): an exact least-squares oracle in Fractions, a record
builder, a copy of the fit whose operators are parameters (for the mutations), and the named cases -- each one cell's integer
triples (u, w, k) with its configuration, the edge it reaches and what the specification intends there.  No GPU, no test
functions: tests/test_slope_fit_cases.py asserts them on the CPU, tests/test_sectors_slope_values_gpu.py runs them on the
device.  The oracle shares nothing with tests/sectors_slope_ref.py; the builder asks that file where a record lands.  The
literal point lists below were found by the seeded searches at the end of this file (python tests/slope_fit_cases.py prints
them again)."""
import math
import operator
from fractions import Fraction

import numpy as np

import sectors_slope_ref as sref

F32 = np.float32
CELL_SIZE, QUANTUM = 0.5, 1.0 / 512.0            # dyadic: steps 1 .. 9 are exact
MAX_SLOPE = 0.26794919                           # the default, tanf(15 degrees)
DEFAULTS = dict(min_count=1, max_spread_q2=625, max_slope=MAX_SLOPE)
EYE, ZERO = np.eye(3), np.zeros(3)


# ---------------------------------------------------------------------------------------------------- the exact oracle
def round_half_even(x):
    """Fraction -> int."""
    f = x.numerator // x.denominator
    r = x - f
    if 2 * r > 1 or (2 * r == 1 and f % 2):
        f += 1
    return f


def nearest_float32(x):
    """The float32 nearest to the Fraction x, ties to even."""
    if x == 0:
        return F32(0.0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    step = Fraction(2) ** (max(e, -126) - 23)
    v = round_half_even(a / step) * step
    out = F32(float(v))
    assert Fraction(float(out)) == v, "out of float32's range"
    return -out if x < 0 else out


def ulps(a, b):
    """The distance of two float32 in units in the last place (+0 and -0 are one value)."""
    def key(x):
        i = int(np.asarray(x, dtype=F32).view(np.int32))
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))


def scale_of(sub, quantum=QUANTUM, cell_size=CELL_SIZE):
    return Fraction(float(F32(quantum))) * (2 * sub) / Fraction(float(F32(cell_size)))


def exact_fit(points, sub=8, min_count=1, max_spread_q2=625, max_slope=MAX_SLOPE, quantum=QUANTUM, cell_size=CELL_SIZE):
    """One cell's (u, w, k) -> the least-squares plane k ~ c + gu u + gw w by Cramer's rule on the 3 x 3 normal equations,
    in Fractions and Python integers, and what the specification intends from it.  u and w count from the cell's centre, so
    c is the plane there."""
    pts = [(int(u), int(w), int(k)) for u, w, k in points]
    n = len(pts)
    su, sw, sk = sum(p[0] for p in pts), sum(p[1] for p in pts), sum(p[2] for p in pts)
    suu, suw, sww = sum(p[0] * p[0] for p in pts), sum(p[0] * p[1] for p in pts), sum(p[1] * p[1] for p in pts)
    suk, swk, skk = sum(p[0] * p[2] for p in pts), sum(p[1] * p[2] for p in pts), sum(p[2] * p[2] for p in pts)

    def det(c0, c1, c2):
        return (c0[0] * (c1[1] * c2[2] - c2[1] * c1[2]) - c1[0] * (c0[1] * c2[2] - c2[1] * c0[2]) + c2[0] * (c0[1] * c1[2] - c1[1] * c0[2]))

    col0, col1, col2, rhs = (n, su, sw), (su, suu, suw), (sw, suw, sww), (sk, suk, swk)
    dm = det(col0, col1, col2)
    A, B, C = n * suu - su * su, n * suw - su * sw, n * sww - sw * sw
    AC, D = A * C, A * C - B * B
    assert D == n * dm, "the determinant of the normal equations is (A C - B B) / N"
    m = sk // n                                                     # the floor mean
    o = dict(n=n, m=m, AC=AC, D=D, su=su, sw=sw, one_minus_rho2=Fraction(D, AC) if AC > 0 else None)
    o["enough"] = n >= max(min_count, 3)
    o["gate"] = AC > 0 and D * (1 << 20) > AC
    o["fitted"] = o["enough"] and o["gate"]
    scale = scale_of(sub, quantum, cell_size)
    if dm != 0:
        c, gu, gw = Fraction(det(rhs, col1, col2), dm), Fraction(det(col0, rhs, col2), dm), Fraction(det(col0, col1, rhs), dm)
        rss = skk - c * sk - gu * suk - gw * swk                    # at the solution: sum of squares of the residuals
        assert rss >= 0
        tilt2 = (gu * scale) ** 2 + (gw * scale) ** 2
        o.update(c=c, gu=gu, gw=gw, rss=rss, c0=c - m, tilt2=tilt2, level_centre=round_half_even(c))
    if o["fitted"]:
        o["slope_a"], o["slope_b"] = nearest_float32(gu * scale), nearest_float32(gw * scale)
        o["level_q"] = m + round_half_even(c - m)                   # the specification's: the tie goes to the even c0
        o["resid_q2"] = min(rss.numerator // (rss.denominator * n), 0xFFFFFFFE)
        o["tilt_ok"] = tilt2 <= Fraction(float(F32(max_slope))) ** 2
        o["resid_ok"] = o["resid_q2"] <= max_spread_q2
        o["flat"] = o["tilt_ok"] and o["resid_ok"]
    else:
        S = skk - 2 * m * sk + n * m * m
        o.update(slope_a=None, slope_b=None, level_q=m, resid_q2=S // n, tilt_ok=False, resid_ok=False, flat=False)
    return o


# ---------------------------------------------------------------------------------------------------- the fit, with its operators
def floor_mean(total, n):
    return total // n


def trunc_mean(total, n):
    return -((-total) // n) if total < 0 else total // n


def rint(x):
    return float(round(x))                       # Python rounds a float half to even


OPS = dict(gate=operator.gt, tilt=operator.le, resid=operator.le, enough=operator.ge, b_sign=1.0, rnd=rint, clamp=lambda q: q if q > 0.0 else 0.0,
           mean=floor_mean, swap=False, scale_factor=lambda sub: 2 * sub, pre_m=lambda m: m)
MUTATIONS = {
    "gate >= for >": dict(gate=operator.ge),
    "tilt < for <=": dict(tilt=operator.lt),
    "resid < for <=": dict(resid=operator.lt),
    "count > for >=": dict(enough=operator.gt),
    "B with the wrong sign": dict(b_sign=-1.0),
    "trunc for rint": dict(rnd=lambda x: float(math.trunc(x))),
    "half up for half to even": dict(rnd=lambda x: float(math.floor(x + 0.5))),
    "the clamp of Q dropped": dict(clamp=lambda q: q),
    "the truncated mean for the floor mean": dict(mean=trunc_mean),
    "gu and gw exchanged": dict(swap=True),
    "scale without the factor 2P": dict(scale_factor=lambda sub: 1),
    "suk', swk' without m": dict(pre_m=lambda m: 0),
}


def fit_copy(points, sub=8, min_count=1, max_spread_q2=625, max_slope=MAX_SLOPE, ops=None):
    """The SLOPE block's fit of one cell in Python floats (IEEE double, one rounding per operation), its decisions and
    roundings taken from `ops`.  With OPS it is the specification; tests/test_slope_fit_cases.py holds it to
    SectorsSlopeRef.cells on every case before it mutates it."""
    op = dict(OPS, **(ops or {}))
    pts = [(int(u), int(w), int(k)) for u, w, k in points]
    n = len(pts)
    isu, isw, isk = sum(p[0] for p in pts), sum(p[1] for p in pts), sum(p[2] for p in pts)
    isuu, isuw, isww = sum(p[0] * p[0] for p in pts), sum(p[0] * p[1] for p in pts), sum(p[1] * p[1] for p in pts)
    isuk, iswk, iskk = sum(p[0] * p[2] for p in pts), sum(p[1] * p[2] for p in pts), sum(p[2] * p[2] for p in pts)
    m = op["mean"](isk, n)
    iS = iskk - 2 * m * isk + n * m * m
    o = dict(fitted=0, slope_a=sref.NOT_FITTED, slope_b=sref.NOT_FITTED, level_q=m, resid_q2=iS // n, flat=0, Q=None, c0=None, sa=None, sb=None)
    N, S, r = float(n), float(iS), float(isk - n * m)
    su, sw, suu, suw, sww = float(isu), float(isw), float(isuu), float(isuw), float(isww)
    suk, swk = float(isuk - op["pre_m"](m) * isu), float(iswk - op["pre_m"](m) * isw)
    A, B, C = N * suu - su * su, op["b_sign"] * (N * suw - su * sw), N * sww - sw * sw
    E, F, G = N * suk - su * r, N * swk - sw * r, N * S - r * r
    AC = A * C
    D = AC - B * B
    if not (op["enough"](n, max(min_count, 3)) and AC > 0.0 and op["gate"](D * 1048576.0, AC)):
        return o
    if D == 0.0:
        return dict(o, fitted=1, slope_a=None)   # (only a mutated gate comes here)
    gu, gw = (E * C - F * B) / D, (F * A - E * B) / D
    if op["swap"]:
        gu, gw = gw, gu
    Q, c0 = (G - gu * E) - gw * F, ((r - gu * su) - gw * sw) / N
    scale = float(F32(QUANTUM)) * float(op["scale_factor"](sub)) / float(F32(CELL_SIZE))
    sa, sb = gu * scale, gw * scale
    rc = min(max(op["rnd"](c0), -2147483648.0), 2147483647.0)
    mq = math.floor(op["clamp"](Q) / (N * N))
    resid = 0xFFFFFFFE if mq >= 4294967294.0 else int(mq) & 0xFFFFFFFF
    flat = op["resid"](resid, max_spread_q2) and op["tilt"](sa * sa + sb * sb, float(F32(max_slope)) * float(F32(max_slope)))
    return dict(fitted=1, slope_a=int(F32(sa).view(np.uint32)), slope_b=int(F32(sb).view(np.uint32)), level_q=m + int(rc), resid_q2=resid,
                flat=int(flat), Q=Q, c0=c0, sa=sa, sb=sb)


# ---------------------------------------------------------------------------------------------------- the record builder
def ref_of(sub=8, n_a=4, n_b=3, **cfg):
    """tests/sectors_slope_ref.py for cells of 0.5 and a quantum of 2^-9 (inv_c = 2, inv_q = 512, both exact); needs no library."""
    c = dict(n_a=n_a, n_b=n_b, cell_size=CELL_SIZE, quantum=QUANTUM, axes=(1, 2, 3), max_step_q=50, window=0, w_dist=1, w_rough=1, rough_cap=65535)
    c.update(DEFAULTS)
    c.update(cfg)
    max_slope = c.pop("max_slope")
    geo = type("Geo", (), dict(inv_c=F32(1.0 / CELL_SIZE), inv_q=F32(1.0 / QUANTUM)))
    return sref.SectorsSlopeRef(type("Cfg", (), c), type("SCfg", (), dict(sub=sub, max_slope=max_slope)), geo)


def build_records(cells, sub, n_a, n_b, origin=(0.0, 0.0, 0.0)):
    """{(i, j): [(u, w, k), ...]} -> (float32 xyz (n, 3), the step's 20 words): every record at the centre of its sub-step,
    its height origin[2] + k quanta.  Asserts, through SectorsSlopeRef.bin, that every record lands where it was meant to."""
    xyz, want = [], []
    for (i, j), pts in cells.items():
        assert 0 <= i < n_a and 0 <= j < n_b
        p = np.asarray(pts, dtype=np.int64).reshape(-1, 3)
        u, w, k = p[:, 0], p[:, 1], p[:, 2]
        a = origin[0] + (i + ((u + sub - 1) / 2 + 0.5) / sub) * CELL_SIZE
        b = origin[1] + (j + ((w + sub - 1) / 2 + 0.5) / sub) * CELL_SIZE
        xyz.append(np.stack([a, b, origin[2] + k * QUANTUM], axis=1))
        want.append(np.stack([np.full(len(p), j * n_a + i), k, u, w], axis=1))
    xyz64, want = np.concatenate(xyz), np.concatenate(want)
    xyz = xyz64.astype(F32)
    assert np.array_equal(xyz.astype(np.float64), xyz64), "a coordinate that float32 does not hold"
    step = sref.step_words(EYE, ZERO, origin)
    part, cell, k, u, w = ref_of(sub=sub, n_a=n_a, n_b=n_b).bin(xyz, step)
    assert part.all() and np.array_equal(np.stack([cell, k, u, w], axis=1), want), "a record that does not land where it was meant to"
    return xyz, step


def layout(n_cases):
    """-> (n_a, n_b, [(i, j), ...]): 4 x 3, or 8 x 8 for more than six cases; every other cell, so that each case's
    neighbours in its row and in its column are empty."""
    n_a, n_b = (4, 3) if n_cases <= 6 else (8, 8)
    at = [(i, j) for j in range(n_b) for i in range(n_a) if (i + j) % 2 == 0]
    assert n_cases <= len(at)
    return n_a, n_b, at[:n_cases]


# ---------------------------------------------------------------------------------------------------- the cases
class Case:
    """One cell: its points, its session's configuration, the edge it reaches and the decisions stated for it."""

    def __init__(self, name, points, edge, sub, cfg, expect):
        self.name, self.family, self.points, self.edge, self.sub = name, name.split("_")[0], [tuple(int(x) for x in p) for p in points], edge, sub
        self.cfg = dict(DEFAULTS, **cfg)
        self.expect = expect

    def exact(self):
        if not hasattr(self, "_exact"):
            self._exact = exact_fit(self.points, sub=self.sub, **self.cfg)
        return self._exact

    def __repr__(self):
        return self.name


CASES = []


def case(name, points, edge, sub=8, expect=None, **cfg):
    assert name not in {c.name for c in CASES} and set(cfg) <= set(DEFAULTS)
    CASES.append(Case(name, points, edge, sub, cfg, expect or {}))
    return CASES[-1]


def by_name(name):
    return next(c for c in CASES if c.name == name)


def family(name):
    return [c for c in CASES if c.family == name]


FAMILIES = ("gate", "tilt", "resid", "level", "thirds", "noise")


def groups(fam):
    """The family's cases by session: [((sub, configuration as sorted items), [cases])], each list one grid of one cloud."""
    out = {}
    for c in family(fam):
        out.setdefault((c.sub, tuple(sorted(c.cfg.items()))), []).append(c)
    return list(out.items())


def grid(us):
    return [(u, w) for w in us for u in us]


ODD8 = tuple(range(-7, 8, 2))

# ---- gate_*: D 2^20 > A C on either side of its threshold, and its degenerate neighbours
def diagonal(n, off):
    """n points at (15, 15), n at (-15, -15) and the off-diagonal ones; heights the gate ignores."""
    return ([(15, 15, 100 + 7 * (i % 5)) for i in range(n)] + [(-15, -15, -40 - 3 * (i % 7)) for i in range(n)] + [(u, w, 11 + 2 * i) for i, (u, w) in enumerate(off)])


case("gate_one_off_holds", diagonal(9320, [(1, -1)]), "N = 18,641: D 2^20 > A C still holds", sub=16, expect=dict(fitted=1))
case("gate_one_off_fails", diagonal(9321, [(1, -1)]), "N = 18,643: D 2^20 > A C fails first", sub=16, expect=dict(fitted=0))
case("gate_two_off_holds", diagonal(18641, [(1, -1), (-1, 1)]), "two off-diagonal points, n = 18,641: the gate holds", sub=16, expect=dict(fitted=1))
case("gate_two_off_fails", diagonal(18642, [(1, -1), (-1, 1)]), "two off-diagonal points, n = 18,642: the gate fails", sub=16, expect=dict(fitted=0))
case("gate_d_zero", [(u, u, 20 + 3 * u) for u in (-15, -9, -3, 1, 7, 13)], "A C > 0 and D == 0 exactly: every point on the diagonal", sub=16,
     expect=dict(fitted=0))
case("gate_a_zero", [(5, w, 9 - 2 * w) for w in (-15, -7, -1, 3, 11)], "A == 0 with C > 0: one u", sub=16, expect=dict(fitted=0))
TRIANGLE = [(-15, -15, 4), (15, -15, 34), (-15, 15, -26), (15, 15, 5), (1, 3, 8), (-7, 9, 2), (11, -5, 19), (3, 3, 7)]
case("gate_count_2_of_3", TRIANGLE[:2], "N = min_fit - 1 = 2 (min_count 1: 3 rules)", sub=16, expect=dict(fitted=0))
case("gate_count_3_of_3", TRIANGLE[:3], "N = min_fit = 3 (min_count 1: 3 rules)", sub=16, expect=dict(fitted=1))
case("gate_count_4_of_3", TRIANGLE[:4], "N = min_fit + 1 = 4 (min_count 1: 3 rules)", sub=16, expect=dict(fitted=1))
case("gate_count_6_of_7", TRIANGLE[:6], "N = min_fit - 1 = 6 (min_count 7)", sub=16, min_count=7, expect=dict(fitted=0))
case("gate_count_7_of_7", TRIANGLE[:7], "N = min_fit = 7 (min_count 7)", sub=16, min_count=7, expect=dict(fitted=1))
case("gate_count_8_of_7", TRIANGLE[:8], "N = min_fit + 1 = 8 (min_count 7)", sub=16, min_count=7, expect=dict(fitted=1))

# ---- tilt_*: sa^2 + sb^2 <= max_tilt2 at equality
AT = float(F32(0.1875))
BELOW, ABOVE = float(np.nextafter(F32(0.1875), F32(0))), float(np.nextafter(F32(0.1875), F32(1)))
ALONG_U = [(u, w, 100 + 3 * u) for u, w in grid(ODD8)]
ALONG_W = [(u, w, -50 - 3 * w) for u, w in grid(ODD8)]
for tag, ms, flat in (("at", AT, 1), ("below", BELOW, 0), ("above", ABOVE, 1)):
    case("tilt_u_%s" % tag, ALONG_U, "sa == 0.1875, gw == 0, max_slope %s 0.1875f" % tag, max_slope=ms, expect=dict(fitted=1, flat=flat))
    case("tilt_w_%s" % tag, ALONG_W, "sb == -0.1875, gu == 0, max_slope %s 0.1875f" % tag, max_slope=ms, expect=dict(fitted=1, flat=flat))
# both components: k = 7 + 4 (u + 2 w) / 3 on multiples of 3 (sub 16): gu = 4/3, gw = 8/3, scale 1/8, so sa^2 + sb^2 = 5/36, which
# no double holds; max_slope is the float32 on either side of sqrt(5)/6 = 0.372677996...
BOTH = [(u, w, 7 + 4 * (u + 2 * w) // 3) for u, w in grid((-15, -9, -3, 3, 9, 15)) if (u, w) != (15, 15)]
BOTH_BELOW = float(F32(math.sqrt(5.0) / 6.0))
if Fraction(BOTH_BELOW) ** 2 > Fraction(5, 36):
    BOTH_BELOW = float(np.nextafter(F32(BOTH_BELOW), F32(0)))
BOTH_ABOVE = float(np.nextafter(F32(BOTH_BELOW), F32(1)))
case("tilt_both_below", BOTH, "sa^2 + sb^2 = 5/36 rounds in double; max_slope the float32 just below sqrt(5)/6", sub=16, max_slope=BOTH_BELOW,
     expect=dict(fitted=1, flat=0))
case("tilt_both_above", BOTH, "sa^2 + sb^2 = 5/36 rounds in double; max_slope the float32 just above sqrt(5)/6", sub=16, max_slope=BOTH_ABOVE,
     expect=dict(fitted=1, flat=1))


# ---- resid_*: resid_q2 <= max_spread_q2 at equality
def twice(d, positions=None):
    """Every position held twice, at +d and -d about k = 40 + 3 u - 2 w: RSS / N == d^2 exactly."""
    return [(u, w, 40 + 3 * u - 2 * w + s * d) for u, w in (positions or grid(ODD8)) for s in (1, -1)]


for d in (1, 25, 181):
    case("resid_d%d_at" % d, twice(d), "RSS / N == %d exactly, max_spread_q2 == %d" % (d * d, d * d), max_spread_q2=d * d, expect=dict(fitted=1, resid_q2=d * d, flat=1))
    case("resid_d%d_under" % d, twice(d), "RSS / N == %d exactly, max_spread_q2 == %d" % (d * d, d * d - 1), max_spread_q2=d * d - 1,
         expect=dict(fitted=1, resid_q2=d * d, flat=0))
QUAD = grid((-7, -3, 3, 7))
# (search_resid_pair: record `out` of twice(25, QUAD) left out, then the height of record `move` moved by dk; RSS / N' lands
# beside an integer, 628 - 0.0021 and 627 + 0.00084)
RESID_JUST = {"below": (2, 24, -3), "above": (10, 1, -2)}


def left_out_and_moved(points, out, move, dk):
    rest = points[:out] + points[out + 1:]
    rest[move] = (rest[move][0], rest[move][1], rest[move][2] + dk)
    return rest


case("resid_just_below", left_out_and_moved(twice(25, QUAD), *RESID_JUST["below"]), "RSS / N = 628 - 6363/3024236, max_spread_q2 == 627", max_spread_q2=627,
     expect=dict(fitted=1, resid_q2=627, flat=1))
case("resid_just_above", left_out_and_moved(twice(25, QUAD), *RESID_JUST["above"]), "RSS / N = 627 + 23/27311, max_spread_q2 == 626", max_spread_q2=626,
     expect=dict(fitted=1, resid_q2=627, flat=0))
# the widest heights: +-29,001 about k = 1 + 400 u - 130 w, every position held 54 times, 37 records left out so that su, sw != 0:
# N S passes 2^53 and G, the products of the gradients and Q all round (r r cannot: 0 <= r < N < 2^23)
WIDE = [(u, w, 1 + 400 * u - 130 * w + (29001 if i % 2 else -29001)) for u, w in grid(ODD8) for i in range(54)][37:]
case("resid_wide", WIDE, "heights +-29,001 about a steep plane, N = 3,419: N S > 2^53, every product of the fit rounds", expect=dict(fitted=1, flat=0))

# ---- level_*: rint(c0) at a half-way value (sub 4, the 4 x 4 positions; search_level).  Each cell is unbalanced, su != 0.
# level_q = m + rint(c0): the tie goes to the even c0, so with an odd m (the first two: 5 - 2 = 3 where c = 3.5, 7 - 0 = 7 where c = 6.5) level_q is the ODD neighbour of the
# plane's centre c = m + c0.
LEVEL_TIES = {
    "m1p5": (Fraction(-3, 2), [(-1, 1, 0), (1, -3, 7), (1, 1, 3), (1, 3, 9), (3, 1, 6)], 5, -2),            # (c0, points, m, rint(c0))
    "m0p5": (Fraction(-1, 2), [(-3, 3, 3), (-1, -1, 7), (1, -1, 6), (1, 3, 12), (3, 1, 8)], 7, 0),
    "p0p5": (Fraction(1, 2), [(-1, -3, 7), (-1, 3, 6), (-1, 3, 8), (1, 1, 3), (3, -3, 8)], 6, 0),
    "p1p5": (Fraction(3, 2), [(-3, -1, 13), (1, 1, 12), (3, -3, 9), (3, -1, 7), (3, 1, 10)], 10, 2),
    "p2p5": (Fraction(5, 2), [(-1, -1, 11), (1, -3, 4), (1, 1, 6), (3, -1, 6), (3, -1, 7)], 6, 2),
}


# A tie in exact arithmetic that the doubles do not keep: c0 == -1.5 exactly, m = 3, so level_q should be 3 - 2 = 1; gu and gw are
# no doubles, the computed c0 falls just above -1.5 and level_q is 2.  (The LEVEL_TIES were searched for an exact computed c0.)
LEVEL_TIE_LOST = [(-3, -1, 1), (1, -3, 13), (1, -1, 1), (1, -1, 3), (3, 3, 0)]


LOST = Case("lost_level_tie", LEVEL_TIE_LOST, "c0 == -3/2 exactly, m = 3; the computed c0 is just above -1.5 and level_q is 2, not 1", 4, {},
            dict(fitted=1))


def one_count_either_side(points):
    """The first point whose height, one quantum up and one down, moves the exact c0 off the tie to either side."""
    tie = exact_fit(points, sub=4)["c"]
    for i in range(len(points)):
        up = [(u, w, k + (j == i)) for j, (u, w, k) in enumerate(points)]
        down = [(u, w, k - (j == i)) for j, (u, w, k) in enumerate(points)]
        cu, cd = exact_fit(up, sub=4), exact_fit(down, sub=4)
        if cu["fitted"] and cd["fitted"] and cd["c"] < tie < cu["c"]:
            return down, up
    raise AssertionError("no such point")


for tag, (c0, pts, m, rc) in LEVEL_TIES.items():
    case("level_%s_tie" % tag, pts, "c0 == %s exactly, m = %d: rint gives %d" % (c0, m, rc), sub=4, expect=dict(fitted=1, level_q=m + rc))
    lo, hi = one_count_either_side(pts)
    case("level_%s_down" % tag, lo, "one height a quantum lower: c0 just below %s" % c0, sub=4, expect=dict(fitted=1, level_q=exact_fit(lo, sub=4)["level_q"]))
    case("level_%s_up" % tag, hi, "one height a quantum higher: c0 just above %s" % c0, sub=4, expect=dict(fitted=1, level_q=exact_fit(hi, sub=4)["level_q"]))
    # every height negative: the floor mean is not the truncated mean and um, uS, s[7] - um s[2] wrap; an even and an odd m
    for name, shift in (("neg", -32000), ("negodd", -32001), ("pos", 32000)):
        case("level_%s_%s" % (tag, name), [(u, w, k + shift) for u, w, k in pts], "c0 == %s exactly, m = %d" % (c0, m + shift), sub=4,
             expect=dict(fitted=1, level_q=m + shift + rc))

# ---- thirds_*: exact planes k = c + s (u + 2 w) / 3 on {+-3, +-9, +-15}^2 (sub 16): RSS == 0, gu = s / 3 is no double, the
# computed Q is a rounding residue (search_thirds: of 2,000 such cells Q < 0 in 80, Q > 0 in 64, Q == 0 in the rest)
THIRDS = {
    "negative": [
        [(-15, -3, -2573), (-15, 9, -3565), (-9, -9, -2325), (-9, 15, -4309), (-3, -3, -3069), (-3, 9, -4061), (-3, 15, -4557), (3, -3, -3317), (3, 3,
         -3813), (3, 15, -4805), (15, -3, -3813), (15, 9, -4805)],
        [(-15, -15, 1578), (-15, -3, 4946), (-15, 3, 6630), (-15, 9, 8314), (-9, -15, 2420), (-3, 9, 9998), (3, -15, 4104), (3, -9, 5788), (9, -9,
         6630), (9, 3, 9998), (15, 9, 12524)],
        [(-9, -3, -5278), (-3, -3, -3390), (-3, 3, 386), (3, -15, -9054), (3, -3, -1502), (9, -15, -7166), (9, -9, -3390), (15, 3, 6050)],
    ],
    "positive": [
        [(-15, -3, -12968), (-15, 15, -2912), (-9, -15, -17996), (-9, 9, -4588), (-3, 15, 440), (9, 3, -2912), (15, -3, -4588), (15, 9, 2116)],
        [(-9, -3, 687), (-9, 9, -6305), (3, -15, 4183), (3, 9, -9801), (15, 3, -9801), (15, 9, -13297)],
        [(-15, -15, -2942), (-15, 9, 3522), (-9, 3, 2714), (-9, 9, 4330), (-3, 15, 6754), (3, -15, -518), (3, -3, 2714), (3, 15, 7562), (9, -3, 3522),
         (15, -15, 1098), (15, 9, 7562)],
    ],
    "zero": [
        [(-15, -9, -5514), (-15, -3, -3950), (-15, 9, -822), (-9, -3, -3168), (-9, 15, 1524), (-3, -15, -5514), (-3, -9, -3950), (-3, 3, -822), (-3,
         9, 742), (9, 9, 2306), (15, -9, -1604)],
        [(-15, -9, -17750), (-15, -3, -12486), (-15, 3, -7222), (-9, -3, -9854), (-9, 3, -4590), (-9, 15, 5938), (-3, 9, 3306), (3, 15, 11202), (15,
         3, 5938), (15, 9, 11202)],
        [(-15, -3, 14764), (-9, -9, 17120), (-9, 15, -1728), (-3, 3, 5340), (-3, 15, -4084), (3, -15, 17120), (3, -3, 7696), (3, 3, 2984), (3, 15,
         -6440), (9, -3, 5340), (15, -15, 12408), (15, 3, -1728)],
    ],
}
for sign, cells in THIRDS.items():
    for i, pts in enumerate(cells):
        case("thirds_%s_%d" % (sign, i), pts, "an exact plane of gradient s / 3: RSS == 0, the computed Q is %s" % sign, sub=16,
             expect=dict(fitted=1, resid_q2=0, q_sign=sign))


# ---- noise_*: seeded random cells for the comparison with exact least squares
def noise_cell(seed, n, sub):
    """n points on random sub-steps with unbalanced coverage, a gradient of up to about 40 degrees, noise of +-3 quanta."""
    rng = np.random.default_rng(seed)
    us = np.arange(-(sub - 1), sub, 2)
    u, w = rng.choice(us, n, p=rng.dirichlet(np.full(sub, 0.7))), rng.choice(us, n, p=rng.dirichlet(np.full(sub, 0.7)))
    rise, way = math.tan(rng.uniform(0.0, math.radians(40.0))), rng.uniform(0.0, 2.0 * math.pi)
    gu, gw = rise * math.cos(way) / float(scale_of(sub)), rise * math.sin(way) / float(scale_of(sub))
    k = np.rint(rng.integers(-2000, 2000) + gu * u + gw * w).astype(np.int64) + rng.integers(-3, 4, n)
    return list(zip(u.tolist(), w.tolist(), k.tolist()))


for sub in (2, 8, 16):
    for n in (3, 17, 64, 1025):
        seed = next(s for s in range(1000 * sub + n, 1000 * sub + n + 100) if exact_fit(noise_cell(s, n, sub), sub=sub)["fitted"])
        case("noise_sub%d_n%d" % (sub, n), noise_cell(seed, n, sub), "seed %d: random positions, a random gradient, noise of a few quanta" % seed, sub=sub,
             expect=dict(fitted=1))


# ---------------------------------------------------------------------------------------------------- the seeded searches
def search_level(seed=1, heights=14):
    """Cells of N <= 8 points on the 4 x 4 positions of sub 4 whose exact c0 is -1.5, -0.5, 0.5, 1.5 and 2.5, su != 0."""
    rng = np.random.default_rng(seed)
    want, found = {-3: None, -1: None, 1: None, 3: None, 5: None}, {}
    pos = np.array(grid((-3, -1, 1, 3)), dtype=np.int64)
    while len(found) < len(want):
        n = int(rng.integers(3, 9))
        idx = rng.integers(0, 16, (200000, n))
        k = rng.integers(0, heights, (200000, n))
        u, w = pos[idx, 0], pos[idx, 1]
        su, sw, sk = u.sum(1), w.sum(1), k.sum(1)
        suu, suw, sww, suk, swk = (u * u).sum(1), (u * w).sum(1), (w * w).sum(1), (u * k).sum(1), (w * k).sum(1)
        dm = n * (suu * sww - suw * suw) - su * (su * sww - suw * sw) + sw * (su * suw - suu * sw)
        dc = sk * (suu * sww - suw * suw) - su * (suk * sww - suw * swk) + sw * (suk * suw - suu * swk)
        m = sk // n
        for t2 in want:
            if t2 in found:
                continue
            hit = np.flatnonzero((dm > 0) & (su != 0) & (2 * (dc - m * dm) == t2 * dm))
            for h in hit:
                pts = sorted(zip(u[h].tolist(), w[h].tolist(), k[h].tolist()))
                e = exact_fit(pts, sub=4)
                # (a tie in exact arithmetic is one in double only where the quotients come out exact: ask for that too)
                if e["fitted"] and e["c0"] == Fraction(t2, 2) and len(set(pts)) == len(pts) and fit_copy(pts, sub=4)["c0"] == t2 / 2.0:
                    found[t2] = pts
                    break
    return {Fraction(t2, 2): found[t2] for t2 in sorted(found)}


def thirds_cell(rng):
    n = int(rng.integers(6, 13))
    at = rng.choice(36, n, replace=False)
    s, c = (3 * int(rng.integers(0, 500)) + int(rng.integers(1, 3))) * int(rng.choice([-1, 1])), int(rng.integers(-9000, 9000))
    g = grid((-15, -9, -3, 3, 9, 15))
    return sorted((g[i][0], g[i][1], c + s * (g[i][0] + 2 * g[i][1]) // 3) for i in at)


def search_thirds(seed=2, tries=2000, each=3):
    """Exact planes k = c + s (u + 2 w) / 3 on {+-3, +-9, +-15}^2: the true RSS is 0, the computed Q a rounding residue."""
    rng = np.random.default_rng(seed)
    signs = {"negative": [], "positive": [], "zero": []}
    for _ in range(tries):
        pts = thirds_cell(rng)
        f = fit_copy(pts, sub=16)
        if not f["fitted"]:
            continue
        signs["negative" if f["Q"] < 0 else "positive" if f["Q"] > 0 else "zero"].append(pts)
    return {k: v[:each] for k, v in signs.items()}, {k: len(v) for k, v in signs.items()}


def search_resid_pair(d=25):
    """The set of `twice(d, QUAD)` with one record left out and one height moved by up to 3: the RSS / N' nearest below and
    nearest above an integer."""
    base = twice(d, QUAD)
    best = {"below": (Fraction(0), None), "above": (Fraction(1), None)}
    for out in range(len(base)):
        rest = base[:out] + base[out + 1:]
        for move in range(len(rest)):
            for dk in (-3, -2, -1, 1, 2, 3):
                pts = list(rest)
                pts[move] = (pts[move][0], pts[move][1], pts[move][2] + dk)
                e = exact_fit(pts)
                q = e["rss"] / e["n"]
                frac = q - (q.numerator // q.denominator)
                if frac == 0:
                    continue
                if frac > best["below"][0]:
                    best["below"] = (frac, pts)
                if frac < best["above"][0]:
                    best["above"] = (frac, pts)
    return best


if __name__ == "__main__":
    for t, pts in search_level().items():
        print("level", t, pts)
    found, counts = search_thirds()
    print("thirds", counts)
    for sign, cells in found.items():
        for pts in cells:
            print("thirds", sign, pts)
    for side, (frac, pts) in search_resid_pair().items():
        print("resid", side, float(frac), pts)
