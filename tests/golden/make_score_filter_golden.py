#!/usr/bin/env python3
"""Known answers for the matching-score pre-filter of MatchingScoreCb1/2 (src/depth_map_fusion.cpp:64-99).

NOT outputs of the reference (it cannot be built here and ships no fixtures): a per-pixel restatement of the chain
in exact rational arithmetic, one rounding per stage --

  * A   = the exact rational (sum t13 t13 F) / 65536 rounded half to even; F read through borderInterpolate
          (REFLECT_101) about the FRAME, the square being a view;
  * M   = 255 when the exact rational 3/100 * (sum d s A) rounds (half to even) above 30, else 0 -- the
          threshold is evaluated from the definition, not from the I >= 1017 shortcut;
  * B   = CV4: (sum t21 t21 M) / 65536 rounded half up; CV3: rounded half to even;
  * out = min(255, S + 2 B).

The tap tables come from tests/score_filter_ref.py (the fp64 derivation) and are stored beside the cases.
Run:  python tests/golden/make_score_filter_golden.py   (pure python + numpy, a few minutes) -> score_filter.npz
"""
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from score_filter_ref import SOBEL_D, SOBEL_S, tap_tables  # noqa: E402


def bi(p, n):  # cv::borderInterpolate, BORDER_REFLECT_101
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def round_even(q: Fraction) -> int:
    f = q.numerator // q.denominator
    r = q - f
    return f + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2) else 0)


def chain(frame, square, direction, form):
    x, y, n = square
    h, w = frame.shape
    t13, t21 = (list(map(int, t)) for t in tap_tables(form))
    F = [[int(v) for v in row] for row in frame]
    A = [[round_even(Fraction(sum(t13[v] * t13[u] * F[bi(y + r + v - 6, h)][bi(x + c + u - 6, w)]
                                  for v in range(13) for u in range(13)), 65536)) for c in range(n)] for r in range(n)]
    kr, kc = (SOBEL_S, SOBEL_D) if direction == 0 else (SOBEL_D, SOBEL_S)  # kr along a row (x), kc along a column
    M = [[0] * n for _ in range(n)]
    for r in range(n):
        for c in range(n):
            i = sum(int(kc[v]) * int(kr[u]) * A[bi(r + v - 3, n)][bi(c + u - 3, n)] for v in range(7) for u in range(7))
            M[r][c] = 255 if round_even(Fraction(3, 100) * i) > 30 else 0
    B = np.zeros((n, n), np.uint8)
    out = np.zeros((n, n), np.uint8)
    for r in range(n):
        for c in range(n):
            q = Fraction(sum(t21[v] * t21[u] * M[bi(r + v - 10, n)][bi(c + u - 10, n)]
                             for v in range(21) for u in range(21)), 65536)
            b = (q + Fraction(1, 2)).numerator // (q + Fraction(1, 2)).denominator if form == 4 else round_even(q)
            B[r, c] = b
            out[r, c] = min(255, F[y + r][x + c] + 2 * b)
    return np.array(A, np.uint8), out, B


def tie_frame(rng):
    """A 40 x 40 frame with a G13 rounding tie (sum = 65536 q + 32768) at square pixel (14, 14) of square (6, 6, 28)."""
    t13, _ = tap_tables(4)
    k = np.outer(t13, t13)
    while True:
        f = rng.integers(0, 256, size=(40, 40)).astype(np.int64)
        win = f[14:27, 14:27]  # the 13 x 13 window of frame pixel (20, 20)
        base = int((k * win).sum()) - k[0, 0] * win[0, 0] - k[0, 1] * win[0, 1] - k[1, 1] * win[1, 1]
        a = np.arange(256)
        tot = base + k[0, 0] * a[:, None, None] + k[0, 1] * a[None, :, None] + k[1, 1] * a[None, None, :]
        hit = np.argwhere(tot % 65536 == 32768)
        if len(hit):
            i, j, m = hit[0]
            f[14, 14], f[14, 15], f[15, 15] = i, j, m
            return f.astype(np.uint8), (6, 6, 28)


def cases():
    rng = np.random.default_rng(20261016)
    land = rng.integers(0, 256, size=(40, 64)).astype(np.uint8)
    yield "landscape_offsets", land, (17, 3, 33)          # inside: G13 reads frame pixels on every side
    yield "landscape_edge_tl", land, (0, 0, 40)           # touches top, bottom and left edges of the frame
    yield "landscape_edge_r", land, (64 - 29, 11, 29)     # touches the right edge only
    yield "const0", np.zeros((24, 30), np.uint8), (3, 2, 20)
    yield "const255", np.full((24, 30), 255, np.uint8), (3, 2, 20)
    yy, xx = np.mgrid[0:40, 0:48]
    yield "hstripes", np.where((yy // 5) % 2 == 0, 230, 20).astype(np.uint8), (4, 1, 37)   # rows alternate
    yield "vstripes", np.where((xx // 5) % 2 == 0, 230, 20).astype(np.uint8), (8, 0, 40)   # columns alternate
    yield "step", np.where(yy < 17, 10, 240).astype(np.uint8), (0, 3, 30)
    yield "tiny", rng.integers(0, 256, size=(11, 14)).astype(np.uint8), (2, 0, 11)  # n = 11: the smallest square
    f, sq = tie_frame(rng)
    yield "g13_tie", f, sq
    from score_patterns import golden_crops  # crops of the value patterns: no blind spot shared by restatement and kernel
    yield from golden_crops()


def main():
    out = {}
    t13, t21_4 = tap_tables(4)
    _, t21_3 = tap_tables(3)
    out["t13"], out["t21_cv4"], out["t21_cv3"] = t13, t21_4, t21_3
    names = []
    for name, frame, sq in cases():
        names.append(name)
        out[f"{name}__frame"] = frame
        out[f"{name}__square"] = np.array(sq, np.int32)
        for direction in (0, 1):
            for form in (4, 3):
                a, o, b = chain(frame, sq, direction, form)
                out[f"{name}__A"] = a  # the same for every direction and form
                out[f"{name}__d{direction}_f{form}__out"] = o
                out[f"{name}__d{direction}_f{form}__grad"] = b
        print(name, flush=True)
    out["names"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "score_filter.npz"), **out)


if __name__ == "__main__":
    main()
