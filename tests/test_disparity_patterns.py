"""CPU side of the range tests of the reprojection: the generators of disparity_patterns.py reach what they say, the
integer form of the exact reference equals the Fraction form the goldens were made with, and the oracle holds its own
bounds against the exact answers over the whole float range.  No GPU."""
import os
from fractions import Fraction

import numpy as np
import pytest

import disparity_patterns as dp
import exact_reproject as ex
import oracle
from helpers import line_bits

SHAPE_NAMES = list(dp.SHAPES)
ALL = [(n, s) for s in SHAPE_NAMES for n in dp.FLOAT_PATTERNS]


def _roi(p, a):
    b = p.border
    h, w = a.shape[-2:]
    return a[..., b:h - b, b:w - b].reshape(a.shape[0], -1)


# ------------------------------------------------------------------------------------------------ the exact reference
def test_integer_form_reproduces_the_committed_goldens(golden_dir):
    g = np.load(os.path.join(golden_dir, "reproject_exact.npz"))
    for name in ("A_default_q_k8", "B_dense_q", "C_extremes", "E_flt_max_sentinel", "E_flt_max_sentinel_dense_q"):
        r = ex.exact_reproject(g[name + "__q"], g[name + "__disp"], int(g[name + "__border"]))
        assert r["has_exact"].all()
        assert np.array_equal(r["bits"][0], g[name + "__expected_bits"]), name


def test_integer_form_equals_the_fraction_form_over_the_float_range():
    """exact_reproject against exact_points (Fraction) on a sample of the sweep's values, and its boundary distance
    against the definition evaluated in Fractions."""
    rng = np.random.default_rng(1)
    vals = dp.sweep_values(rng).view(np.float32)
    vals = vals[np.isfinite(vals) & (vals != 0)]
    disp = rng.permutation(vals)[:24 * 40].reshape(24, 40)
    for q in (dp.rig_q(40, 24), dp.w_zero_sliver(1, "ragged", 2).q, dp.near_integer_cx_q("ragged")):
        r = ex.exact_reproject(q, disp, 0)
        assert r["has_exact"].all()
        want = ex.exact_points(q, disp, 0)
        # (a zero NUMERATOR -- v + cy == 0 in the middle row -- is +0 in the Fraction form and takes W's sign here)
        zero_num = np.zeros(want.shape, dtype=bool)
        zero_num[:, 1] = (np.repeat(np.arange(24), 40) + q[7]) == 0
        want[zero_num & (r["bits"][0] == 0x80000000)] |= 0x80000000
        assert np.array_equal(r["bits"][0], want)
    # the distance: |x - nearest boundary| / |x| with the boundaries taken from the float32 grid itself
    q = dp.rig_q(40, 24)
    r = ex.exact_reproject(q, disp, 0)
    qf = [Fraction(float(v)) for v in q]
    checked = 0
    for i in rng.permutation(disp.size)[:150]:
        v, u = divmod(int(i), 40)
        x = (qf[0] * u + qf[3]) / (qf[14] * Fraction(float(disp[v, u])) + qf[15])
        got = np.uint32(r["bits"][0, i, 0]).view(np.float32)
        if not np.isfinite(got) or x == 0:
            continue
        nb = [np.nextafter(got, np.float32(-np.inf)), np.nextafter(got, np.float32(np.inf))]
        bounds = [(Fraction(float(got)) + (Fraction(float(n)) if np.isfinite(n) else Fraction(float(got)) * 2 - Fraction(float(nb[0])))) / 2
                  for n in nb]
        want = min(abs(x - b) for b in bounds) / abs(x)
        assert abs(Fraction(r["dist"][0, i, 0]) - want) <= want * Fraction(1, 2 ** 50), (u, v)
        checked += 1
    assert checked > 100


def test_rounding_at_the_edges_of_the_range():
    T = ex.OVERFLOW_THRESHOLD
    assert ex.round_ratio_to_f32(T, 1) == (ex.INF_BITS, 0.0)                     # the tie goes to inf
    assert ex.round_ratio_to_f32(T * 8 - 1, 8)[0] == ex.FLT_MAX_BITS
    assert ex.round_ratio_to_f32(-T, 1)[0] == 0xFF800000
    assert ex.round_ratio_to_f32(1, 2 ** 150)[0] == 0                            # the tie at half the smallest subnormal: to even
    assert ex.round_ratio_to_f32(3, 2 ** 151)[0] == 1
    assert ex.round_ratio_to_f32(-3, 2 ** 150)[0] == 0x80000002                  # 1.5 subnormal ulps: tie to even
    assert ex.round_ratio_to_f32(2 ** 24 - 1, 2 ** 150)[0] == 0x00800000         # rounds up into the first normal binade
    assert ex.round_ratio_to_f32(0, -5, zero_negative=True) == (0x80000000, float("inf"))
    assert ex.round_ratio_to_f32(1, 3)[0] == ex.f32_bits(float(np.float32(1 / 3)))


# ------------------------------------------------------------------------------- each generator reaches what it says
@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_binade_sweep_reaches_every_binade_at_the_promised_columns(shape):
    p = dp.with_exact("binade_sweep", shape)
    w, h, border, _ = dp.SHAPES[shape]
    bits = p.frames.view(np.uint32)
    assert len(p.promised) == 4 and all(border <= c < w - border for c in p.promised)
    pc = dp.principal_cols(p.q, w, border)
    assert (pc[0] + p.q[3]) * (pc[1] + p.q[3]) < 0 and abs(pc[1] + p.q[3]) < 2e-3
    cy = p.q[7]
    for c in p.promised:
        col = bits[:, border:h - border, c].reshape(-1)
        fin = col[(col & 0x7FFFFFFF != 0) & (col & 0x7FFFFFFF < 0x7F800000)]
        for sign in (0, 0x80000000):
            e = dp.f32_exponent(fin[(fin & 0x80000000) == sign])
            assert set(range(-149, 128)) <= set(e.tolist()), f"column {c}, sign {sign:#x}"
        assert set(p.values.tolist()) <= set(col.tolist()), f"column {c} misses values"
    # every value on both sides of cy
    side = np.sign(p.placed[:, 1] + cy)
    for s in (-1, 1):
        assert len(np.unique(p.placed[side == s, 3])) == len(p.values)
    for special in (0, 0x80000000, 0x00800000, 0x007FFFFF, 0x7F7FFFFF, 0x7F7FFFFE, 0x7F800000, 0xFF800000, 0x7FC00000, 1, 0x80000001):
        assert special in p.values
    # what the values lead to: subnormal and zero X next to the principal point, overflowed Z, no exact answer for the specials
    xb = p.exact["bits"][..., 0] & 0x7FFFFFFF
    assert ((xb > 0) & (xb < 0x00800000)).sum() >= 100, "subnormal X"
    zb = p.exact["bits"][..., 2]
    assert (zb == 0x7F800000).sum() >= 500 and (zb == 0xFF800000).sum() >= 500
    assert (zb == ex.BIG_Z_BITS).sum() >= 4
    cols_per_value = len(p.placed) // len(p.values)
    assert cols_per_value == 6 and len(p.placed) == 6 * len(p.values)
    assert (~p.exact["has_exact"]).sum() == 5 * cols_per_value   # +-0, +-inf and NaN, once in each of a value's columns


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("q33", ["0.37", "-1/3"])
def test_w_zero_ordinary_changes_sign_far_above_the_sliver(shape, q33):
    p = dp.with_exact("w_zero_ordinary_" + q33, shape)
    w, h, border, _ = dp.SHAPES[shape]
    ws = p.exact["w_sign"]
    on = np.zeros(p.frames.shape, dtype=bool)
    on[p.placed[:, 0], p.placed[:, 1], p.placed[:, 2]] = True
    on = _roi(p, on)
    assert (ws[on] > 0).sum() >= 300 and (ws[on] < 0).sum() >= 300          # ~80 values either side x 6 columns
    assert p.exact["has_exact"].all()                                       # W is never exactly zero
    aw = np.abs(_roi(p, dp.w_values(p)))
    safe = dp.w_safe(p.q, w, h, border)
    assert 2.0 ** -117 < safe < 2.0 ** -116
    assert 0 < aw.min() < 2.0 ** -23 and aw.min() > 2.0 ** 80 * safe        # cancels to ~a ulp(d); no sliver pixel


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("rig", [0, 1, 2])
def test_w_zero_sliver_mixes_the_three_predicate_classes(shape, rig):
    p = dp.with_exact(f"w_zero_sliver_{rig}", shape)
    w, h, border, _ = dp.SHAPES[shape]
    W = _roi(p, dp.w_values(p))[0]
    safe = dp.w_safe(p.q, w, h, border)
    zero, sliver, big = W == 0, (W != 0) & (np.abs(W) < safe), np.abs(W) >= safe
    assert np.array_equal(zero, ~p.exact["has_exact"][0])                   # (the float64 W is exact: the classes are too)
    assert np.array_equal(np.sign(W).astype(np.int8), p.exact["w_sign"][0])
    n = W.size
    assert zero.sum() >= 100 and sliver.sum() >= 0.2 * n and big.sum() >= 0.05 * n, (zero.sum(), sliver.sum(), big.sum())
    assert (W[sliver] > 0).sum() >= 0.05 * n and (W[sliver] < 0).sum() >= 0.05 * n
    # inside the sliver the real arithmetic decides, both ways
    inf = (p.exact["bits"][0, :, :3] & 0x7FFFFFFF) == 0x7F800000
    valid = ~inf.any(axis=1)
    assert (sliver & valid).sum() >= 0.05 * n and (sliver & ~valid).sum() >= 0.05 * n
    assert valid[big].all()                                                 # what w_safe promises
    # ... and the classes alternate inside the kernels' 2,048-pixel tiles
    tiles = [slice(i, i + 2048) for i in range(0, n - 2047, 2048)]
    mixed = sum(1 for t in tiles if zero[t].any() and big[t].any() and (sliver[t] & valid[t]).any() and (sliver[t] & ~valid[t]).any())
    assert mixed >= 0.5 * len(tiles), (mixed, len(tiles))
    # valid and invalid one ulp of d apart
    d = _roi(p, p.frames)[0].view(np.uint32).astype(np.int64)
    vb, ib = np.unique(d[valid & ~zero]), np.unique(d[~valid & ~zero])
    assert np.intersect1d(vb + 1, ib).size + np.intersect1d(vb - 1, ib).size >= 2
    if rig == 2:   # f = 2: X or Y decides where Z is finite
        assert (~inf[:, 2] & (inf[:, 0] | inf[:, 1])).sum() >= 0.05 * n


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("name", ["overflow_edge", "overflow_edge_near_integer_cx"])
def test_overflow_edge_straddles_every_threshold(shape, name):
    p = dp.with_exact(name, shape)
    w, h, border, _ = dp.SHAPES[shape]
    rw = w - 2 * border
    idx = (p.placed[:, 1] - border) * rw + (p.placed[:, 2] - border)
    bits = p.exact["bits"][0, idx]
    d = p.frames.view(np.uint32)[0, p.placed[:, 1], p.placed[:, 2]].astype(np.int64)
    seen = {}
    for g, (coord, edge, _) in enumerate(p.groups):
        sel = p.placed[:, 3] == g
        mag = (bits[sel, coord] & 0x7FFFFFFF).astype(np.int64)
        dd = d[sel]
        lo, hi = {"overflow": (mag < 0x7F800000, mag == 0x7F800000),
                  "min_normal": (mag < 0x00800000, mag >= 0x00800000),
                  "half_min_subnormal": (mag == 0, mag > 0)}[edge]
        assert lo.any() and hi.any(), (g, coord, edge)
        gap = np.abs(dd[lo][:, None] - dd[hi][None, :]).min()
        assert gap <= 2, (g, coord, edge, gap)
        seen[(coord, edge)] = seen.get((coord, edge), 0) + 1
    assert seen[(0, "overflow")] >= 8 and seen[(1, "overflow")] >= 8 and seen[(2, "overflow")] >= 8
    assert seen[(0, "min_normal")] >= 2
    # |X| = 2^-150 needs |u + cx| < a FLT_MAX 2^-150 ~ 2.6e-6: out of the reference rig's reach (5e-4), reached with
    # the principal point 2^-21 from a pixel centre
    assert ((0, "half_min_subnormal") in seen) == (name == "overflow_edge_near_integer_cx")


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_all_raw_values_sit_inside_the_roi(shape):
    w, h, border, _ = dp.SHAPES[shape]
    tiny = float(np.finfo(np.float32).tiny)
    for p, n in ((dp.u16_all_values(3, shape), 65536), (dp.u8_all_values(3, shape), 256)):
        roi = _roi(p, p.frames)[0]
        assert len(np.unique(roi)) == n
        assert np.array_equal(p.frames[0, p.placed[:, 1], p.placed[:, 2]], np.arange(n))
        assert all(float(np.float32(s)) == s for s in p.scales)
        sub, over = dp.decode(roi, p.scales[3]), dp.decode(roi, p.scales[4])
        assert ((sub > 0) & (sub < tiny)).any() and (sub >= tiny).any()
        assert np.isinf(over).any() and np.isfinite(over[roi > 0]).any()
        full = np.float32(p.scales[2]).view(np.uint32)
        assert bin(int(full) & 0x7FFFFF).count("1") >= 8   # a mantissa of many bits: raw * scale rounds for most raw values


@pytest.mark.parametrize("name,shape", ALL)
def test_bit_equality_mask_leaves_out_at_most_a_thousandth(name, shape):
    """The GPU test asserts bit equality with the exact value where bit_equal_mask holds; it may not become vacuous."""
    p = dp.with_exact(name, shape)
    have = p.exact["has_exact"]
    kept = dp.bit_equal_mask(p.exact)
    assert have.sum() >= 0.99 * have.size
    assert (have & ~kept).sum() <= 0.001 * have.sum(), ((have & ~kept).sum(), have.sum())
    # ... nor leave out what the pattern was built for: nearly all the pixels laid down on purpose stay in
    on = np.zeros(p.frames.shape, dtype=bool)
    on[p.placed[:, 0], p.placed[:, 1], p.placed[:, 2]] = True
    on = _roi(p, on) & have
    assert (on & kept).sum() >= 0.95 * on.sum()


# ------------------------------------------------------------------------------------------ the oracle on the patterns
def _line_distance(got, want_bits):
    """|position of got - position of the exact float| on ulp_distance's integer line, inf being the float after FLT_MAX."""
    return np.abs(line_bits(got) - line_bits(want_bits))


def away_from_cancellation(p):
    """|W| >= 2^-20 |a d|: the named forms form W as b + RN(a d), an absolute error of up to 2^-53 (|a d| + |W|), so
    W is then good to 2^-32 relative, 2^-8 of a float32 ulp, and the forms' own bounds (one cast: 1 ulp; a cast of
    the numerator and one of the quotient: 2 ulp) hold.  Closer to the pole of an ordinary rig they do not, as
    include/d2pc.h says of the named forms.  (The sliver mix has no such zone: its a has one or two bits, so a d, b and
    their sum a (d - d0) are all exact in double.)"""
    if getattr(p, "d0", None) is not None:
        return np.ones(p.exact["has_exact"].shape, dtype=bool)
    d = _roi(p, p.frames.astype(np.float64))
    with np.errstate(invalid="ignore"):
        return np.abs(_roi(p, dp.w_values(p))) >= 2.0 ** -20 * np.abs(float(p.q[14]) * d)


@pytest.mark.parametrize("name,shape", ALL)
def test_oracle_forms_against_the_exact_answers(name, shape):
    p = dp.with_exact(name, shape)
    ok = p.exact["has_exact"] & away_from_cancellation(p)
    assert ok.sum() >= 0.99 * ok.size
    for form, bound in ((oracle.FORM_CV24, 1), (oracle.FORM_CV4, 2)):
        for f in range(len(p.frames)):
            got = oracle.reproject(p.frames[f], p.q, border=p.border, form=form)
            assert np.array_equal(got[:, 3].view(np.uint32), p.exact["bits"][f, :, 3])
            m = ok[f]
            assert not np.isnan(got[m, :3]).any(), f"form {form}, frame {f}: NaN where an exact answer exists"
            dist = _line_distance(got[m, :3], p.exact["bits"][f][m, :3])
            assert dist.max() <= bound, f"form {form}, frame {f}: {dist.max()} ulp"
            # where the exact answer is a zero (a zero numerator, or a quotient below 2^-150) the form's is the same
            # zero, sign included
            want = p.exact["bits"][f][m, :3]
            z = (want & 0x7FFFFFFF) == 0
            assert np.array_equal(got[m, :3].view(np.uint32)[z], want[z]), f"form {form}, frame {f}: zeros"


@pytest.mark.parametrize("name,shape", ALL)
@pytest.mark.parametrize("form", [oracle.FORM_CV24, oracle.FORM_CV4])
def test_oracle_compact_is_the_filtered_reprojection(name, shape, form):
    p = dp.make(name, shape)
    w, h, border, _ = dp.SHAPES[shape]
    v, u = np.mgrid[border:h - border, border:w - border]
    pix = (v * w + u).reshape(-1).astype(np.uint32)
    pool = np.unique(p.frames[np.isfinite(p.frames)])
    floors = [-np.inf, float(pool[len(pool) // 2])]
    for f in range(len(p.frames)):
        full = oracle.reproject(p.frames[f], p.q, border=border, form=form)
        d = p.frames[f, border:h - border, border:w - border].reshape(-1)
        for dmin in floors:
            keep = np.isfinite(full[:, :3]).all(axis=1) & ~(d <= np.float32(dmin))
            pts, idx = oracle.reproject_compact(p.frames[f], p.q, border=border, form=form, min_disparity=dmin)
            assert np.array_equal(idx, pix[keep])
            assert np.array_equal(pts.view(np.uint32), full[keep].view(np.uint32))
        assert 0 < keep.sum() < keep.size


@pytest.mark.parametrize("kind,shape", [("u16", "ragged"), ("u8", "border0"), ("u16", "native"), ("u8", "native")])
def test_oracle_decode_over_every_raw_value(kind, shape):
    """(float)raw * scale in the oracle: bit-identical to the decoded frame fed as fp32, for every raw value and scale;
    at the small shapes also against the exact answers."""
    p = (dp.u16_all_values if kind == "u16" else dp.u8_all_values)(3, shape)
    raw = p.frames[0]
    for scale in p.scales:
        d = dp.decode(raw, scale)
        for form, bound in ((oracle.FORM_CV24, 1), (oracle.FORM_CV4, 2)):
            a = oracle.reproject(raw, p.q, border=p.border, scale=scale, form=form)
            b = oracle.reproject(d, p.q, border=p.border, form=form)
            nan = np.isnan(b)
            assert np.array_equal(nan, np.isnan(a)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]), scale
            if shape != "native":
                e = ex.exact_reproject(p.q, d, p.border)
                m = e["has_exact"][0]
                assert _line_distance(a[m, :3], e["bits"][0][m, :3]).max() <= bound, (scale, form)


def test_constant_cells_carry_every_byte_through_a_3x3_median():
    w, h, border, _ = dp.SHAPES["native"]
    img, centre = dp.constant_cells(np.random.default_rng(5), h, w, border, 3)
    assert len(np.unique(img[centre])) == 256
    assert np.array_equal(oracle.median_u8(img, 3)[centre], img[centre])
