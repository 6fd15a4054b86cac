"""The matching-score pre-filter's spec on the CPU: the integer restatement
(tests/score_filter_ref.py) against a per-pixel brute force and the exact-rational golden vectors, the tap tables,
the threshold equivalence round(0.03 I) > 30 <=> I >= 1017 under float32 emulations of OpenCV's Sobel, and the
descriptor defaults of the C ABI."""
import ctypes
import os

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import score_filter_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_filter.npz")


# ---- tap tables -----------------------------------------------------------------------------------------------
def test_tap_tables_sums_and_known_values():
    t13, t21_4 = ref.tap_tables(4)
    t13_3, t21_3 = ref.tap_tables(3)
    assert np.array_equal(t13, t13_3)  # G13: the general path in both generations
    assert t13.tolist() == [5, 9, 14, 21, 28, 33, 35, 33, 28, 21, 14, 9, 5] and t13.sum() == 255
    assert t21_4.tolist() == [9, 9, 11, 11, 12, 13, 13, 14, 14, 15, 14, 15, 14, 14, 13, 13, 12, 11, 11, 9, 9]
    assert t21_4.sum() == 256
    assert t21_3.tolist() == [9, 10, 10, 11, 12, 13, 13, 14, 14, 14, 14, 14, 14, 14, 13, 13, 12, 11, 10, 10, 9]
    assert t21_3.sum() == 254
    for t in (t13, t21_4, t21_3):
        assert np.array_equal(t, t[::-1]) and t.max() <= 36


def test_tap_rounding_margins():
    """Every tap lies far enough from its rounding boundary that softdouble vs libm exp or float vs double casts
    cannot move it: G13 >= 0.079/256, G21 (3.2) one tap at 0.0028/256, G21 (4.x, error-diffused) >= 0.01/256."""
    _, m13 = ref.general_taps(ref.gauss_bitexact(13, 3.0))
    _, m13_3 = ref.general_taps(ref.gauss_cv3(13, 3.0))
    _, m21_3 = ref.general_taps(ref.gauss_cv3(21, 10.0))
    _, m21_4 = ref.fixed_point_taps(ref.gauss_bitexact(21, 10.0))
    assert m13.min() > 0.079 and m13_3.min() > 0.079
    assert 0.0027 < m21_3.min() < 0.0029  # the near-tie of the 3.2 table (taps 2 and 18)
    assert m21_4.min() > 0.01
    # the float kernel of either generation gives the same general-path taps
    assert np.array_equal(ref.general_taps(ref.gauss_bitexact(21, 10.0))[0], ref.general_taps(ref.gauss_cv3(21, 10.0))[0])


def test_constant_frames():
    """Taps summing to 255: a constant 255 frame blurs to 253 after G13 (and the Sobel of a constant is 0)."""
    for v, want_a in ((0, 0), (255, 253), (128, 127)):
        st = ref.stages(np.full((20, 25), v, np.uint8), (2, 1, 19), 0)
        assert (st["A"] == want_a).all() and (st["I"] == 0).all() and (st["B"] == 0).all()
        assert (st["out"] == v).all()


# ---- brute force ----------------------------------------------------------------------------------------------
def _brute(frame, square, direction, form):
    """Per-pixel loops, borderInterpolate per access, threshold from the float definition in exact arithmetic."""
    from fractions import Fraction

    def bi(p, n):
        while p < 0 or p >= n:
            p = -p if p < 0 else 2 * (n - 1) - p
        return p

    x, y, n = square
    h, w = frame.shape
    t13, t21 = ref.tap_tables(form)
    A = np.zeros((n, n), np.int64)
    for r in range(n):
        for c in range(n):
            s = sum(int(t13[v]) * int(t13[u]) * int(frame[bi(y + r + v - 6, h), bi(x + c + u - 6, w)])
                    for v in range(13) for u in range(13))
            q, rem = divmod(s, 65536)
            A[r, c] = q + (rem > 32768 or (rem == 32768 and q % 2))
    kr, kc = (ref.SOBEL_S, ref.SOBEL_D) if direction == 0 else (ref.SOBEL_D, ref.SOBEL_S)
    M = np.zeros((n, n), np.int64)
    for r in range(n):
        for c in range(n):
            i = sum(int(kc[v]) * int(kr[u]) * int(A[bi(r + v - 3, n), bi(c + u - 3, n)]) for v in range(7) for u in range(7))
            val = Fraction(3, 100) * i
            fl = val.numerator // val.denominator
            rnd = fl + (val - fl > Fraction(1, 2) or (val - fl == Fraction(1, 2) and fl % 2))
            M[r, c] = 255 if rnd > 30 else 0
    out = np.zeros((n, n), np.uint8)
    B = np.zeros((n, n), np.uint8)
    for r in range(n):
        for c in range(n):
            s = sum(int(t21[v]) * int(t21[u]) * int(M[bi(r + v - 10, n), bi(c + u - 10, n)])
                    for v in range(21) for u in range(21))
            q, rem = divmod(s, 65536)
            b = q + (rem >= 32768) if form == 4 else q + (rem > 32768 or (rem == 32768 and q % 2))
            B[r, c] = b
            out[r, c] = min(255, int(frame[y + r, x + c]) + 2 * b)
    return out, B


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("form", [4, 3])
def test_restatement_matches_brute_force(direction, form):
    rng = np.random.default_rng(100 + 10 * direction + form)
    # smooth-ish frames so that the threshold goes both ways
    base = rng.integers(0, 256, size=(4, 5)).astype(np.float64)
    frame = np.kron(base, np.ones((5, 5)))[:17, :23]
    frame = np.clip(frame + rng.integers(-20, 21, size=frame.shape), 0, 255).astype(np.uint8)
    for sq in ((0, 0, 17), (5, 2, 13), (12, 6, 11)):
        want_o, want_b = _brute(frame, sq, direction, form)
        got_o, got_b = ref.score_filter(frame, sq, direction, form)
        assert np.array_equal(got_o, want_o), sq
        assert np.array_equal(got_b, want_b), sq
        assert ref.stages(frame, sq, direction, form)["M"].any() or sq[2] == 11


def test_restatement_matches_golden():
    g = np.load(GOLDEN)
    assert np.array_equal(g["t13"], ref.tap_tables(4)[0])
    assert np.array_equal(g["t21_cv4"], ref.tap_tables(4)[1]) and np.array_equal(g["t21_cv3"], ref.tap_tables(3)[1])
    for name in g["names"]:
        frame, sq = g[f"{name}__frame"], tuple(int(v) for v in g[f"{name}__square"])
        assert np.array_equal(ref.stages(frame, sq, 0)["A"], g[f"{name}__A"]), name
        for direction in (0, 1):
            for form in (4, 3):
                o, b = ref.score_filter(frame, sq, direction, form)
                assert np.array_equal(o, g[f"{name}__d{direction}_f{form}__out"]), (name, direction, form)
                assert np.array_equal(b, g[f"{name}__d{direction}_f{form}__grad"]), (name, direction, form)


def test_golden_covers_the_cases_it_claims():
    g = np.load(GOLDEN)
    assert (g["const255__A"] == 253).all() and (g["const0__A"] == 0).all()
    # the stripes cross the threshold in the direction that sees them, and only there
    assert g["hstripes__d0_f4__grad"].max() > 0 and g["vstripes__d1_f4__grad"].max() > 0
    assert g["hstripes__d1_f4__grad"].max() == 0 and g["vstripes__d0_f4__grad"].max() == 0
    # the G13 tie: the exact sum at square pixel (14, 14) is 65536 q + 32768
    t13 = ref.tap_tables(4)[0]
    f = g["g13_tie__frame"].astype(np.int64)
    s = int((np.outer(t13, t13) * f[14:27, 14:27]).sum())
    assert s % 65536 == 32768 and g["g13_tie__A"][14, 14] == ref.rint_even_16(s)
    # the forms differ somewhere
    assert any(not np.array_equal(g[f"{n}__d0_f4__grad"], g[f"{n}__d0_f3__grad"]) for n in g["names"])


# ---- threshold equivalence --------------------------------------------------------------------------------------
def _cv_sobel_f32(tiles, direction, fma):
    """OpenCV's Sobel(., -1, dx, dy, 7, 0.03) on 8-bit 7 x 7 tiles, centre value, in float32: the scale lands on the
    kernel along x when dx == 0 (direction 0) and on the kernel along y otherwise, as float32(k * 0.03); the row pass
    (RowFilter 8u -> 32f) accumulates left to right, the column pass (SymmColumnFilter 32f -> 8u) pairs the symmetric
    rows first.  fma: every multiply-add rounded once (float64, then float32), else product and sum rounded apart."""
    f32 = np.float32
    s, d = ref.SOBEL_S.astype(np.float64), ref.SOBEL_D.astype(np.float64)
    kx, ky = (s * 0.03, d) if direction == 0 else (d, s * 0.03)
    kx, ky = kx.astype(f32), ky.astype(f32)
    a = tiles.astype(f32)

    def mac(acc, k, v):
        if fma:
            return (acc.astype(np.float64) + np.float64(k) * v.astype(np.float64)).astype(f32)
        return (acc + f32(k) * v).astype(f32)

    rows = np.zeros(tiles.shape[:2], f32)  # (tiles, 7 rows)
    for u in range(7):
        rows = mac(rows, kx[u], a[:, :, u])
    col = (f32(ky[3]) * rows[:, 3]).astype(f32)
    for k in range(1, 4):
        col = mac(col, ky[3 + k], (rows[:, 3 + k] + rows[:, 3 - k]).astype(f32))
    return np.rint(col.astype(np.float64))  # cvRound (half to even) before the saturating cast


def _integer_i(tiles, direction):
    kr, kc = (ref.SOBEL_S, ref.SOBEL_D) if direction == 0 else (ref.SOBEL_D, ref.SOBEL_S)
    return np.einsum("v,u,tvu->t", kc, kr, tiles.astype(np.int64))


@pytest.mark.parametrize("direction", [0, 1])
def test_threshold_equivalence(direction):
    rng = np.random.default_rng(7 + direction)
    kr, kc = (ref.SOBEL_S, ref.SOBEL_D) if direction == 0 else (ref.SOBEL_D, ref.SOBEL_S)
    w = np.outer(kc, kr)
    tiles = [rng.integers(0, 256, size=(200000, 7, 7)),
             rng.integers(0, 2, size=(20000, 7, 7)) * 255]          # binary tiles
    # tiles with I in {1015 .. 1018}: a weight-1 corner absorbs the difference
    t = rng.integers(0, 256, size=(40000, 7, 7))
    i = _integer_i(t, direction)
    target = 1015 + (np.arange(len(t)) % 4)
    corner = t[:, 0, 0] + (target - i)  # w[0, 0] == 1
    keep = (corner >= 0) & (corner <= 255)
    t[:, 0, 0] = np.clip(corner, 0, 255)
    tiles.append(t[keep])
    assert w[0, 0] == 1 and keep.sum() > 100
    # the largest |I| either way
    tiles.append(np.stack([np.where(w > 0, 255, 0), np.where(w < 0, 255, 0)]))
    tiles = np.concatenate(tiles).astype(np.uint8)
    ii = _integer_i(tiles, direction)
    assert set(range(1015, 1019)) <= set(ii.tolist())
    want = ii >= ref.THRESHOLD_I
    for fma in (False, True):
        got = _cv_sobel_f32(tiles, direction, fma) > 30
        assert np.array_equal(got, want), (fma, ii[got != want][:10])
    assert np.abs(0.03 * ii - 30.5).min() > 0.0099  # no integer I lands on the rounding boundary (1016, 1017: 0.02, 0.01)


# ---- C ABI descriptor ---------------------------------------------------------------------------------------------
def test_score_filter_desc_init_defaults():
    d = d2pc.score_filter_desc_init()
    assert d.struct_size == ctypes.sizeof(d2pc.ScoreFilterDesc)
    assert (d.direction, d.form, d.n_frames) == (0, d2pc.SCORE_FORM_CV4, 1)
    assert (d.width, d.height, d.x, d.y, d.n) == (0, 0, 0, 0, 0)
    assert not d.src and not d.out and not d.grad
    assert (d.src_pitch, d.out_pitch, d.grad_pitch, d.src_frame_stride) == (0, 0, 0, 0)
    assert (d2pc.SCORE_FORM_CV4, d2pc.SCORE_FORM_CV3) == (4, 3)
