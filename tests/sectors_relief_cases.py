"""Planted frame tables for the relief tests (tests/test_sectors_relief_cpu.py, tests/test_sectors_relief_gpu.py): per-cell
point sets (odd u and w in range, integer k) laid on a synthetic WORLD, so that frames taken at different corners see the same
ground and a window's cell is one plane seen several times.  A world cell's kind and plane come from a hash of its world
index: gentle planes with and without noise (fitted and flat), steep planes (fitted, not flat), rubble (fitted, rough), and
slivers -- one column of positions -- that one frame cannot fit.  The sums are formed here from the points, directly."""
import numpy as np

import sectors_ground_ref as gref

F32 = np.float32
OFF = 0xFFFFFFFF
QUANTUM, CELL = 1.0 / 512.0, 0.5                # scale = 2^-9 * 16 / 0.5 = 0.0625 for sub 8: 4 quanta per half sub-step is 0.25
JUDGE = dict(cell_size=CELL, quantum=QUANTUM, min_count=4, max_spread_q2=200, max_step_q=40, w_dist=2, w_rough=1)
EYE, ZERO = np.eye(3), np.zeros(3)


def corner_step(ia, jb, h0=1.0, goal=(OFF, OFF), cell=CELL):
    return gref.step_words(EYE, ZERO, [cell * ia, cell * jb, h0], *goal)


def sums_of(n, cell, k, u, w):
    """(count uint32, sum int64, sum2 uint64, moments int64 (7 n)) of points given by cell, k, u, w."""
    cell, k, u, w = [np.asarray(x, dtype=np.int64) for x in (cell, k, u, w)]

    def total(term):
        t = np.zeros(n, dtype=np.int64)
        np.add.at(t, cell, term)
        return t

    mom = [total(x) for x in (u, w, u * u, u * w, w * w, u * k, w * k)]
    return np.bincount(cell, minlength=n).astype(np.uint32), total(k), total(k * k).astype(np.uint64), np.concatenate(mom)


def world_kind(wi, wj):
    """kind 0 gentle, 1 gentle with noise, 2 steep, 3 rubble, 4 sliver; and the plane (c, gu, gw) of world cells (wi, wj)."""
    h = ((wi * 73856093) ^ (wj * 19349663)) & 0xFFFFFF
    pick = h % 100
    kind = np.where(pick < 55, 0, np.where(pick < 80, 1, np.where(pick < 87, 2, np.where(pick < 94, 3, 4))))
    gu, gw = (h >> 8) % 5 - 2, (h >> 12) % 5 - 2          # -2 .. 2 quanta per half sub-step: at most 0.177 of tilt, flat
    gu = np.where(kind == 2, 6, gu)                       # 0.375: steeper than tan 15 degrees
    c = 100 + (wi + 2 * wj) % 4
    return kind, c, gu, gw


def frame_points(rng, n_a, n_b, ia, jb, sub=8, fill=0.9, most=10):
    """The points of one frame whose corner is world cell (ia, jb): (cell, k, u, w), 0 .. `most` points per cell."""
    n = n_a * n_b
    j, i = np.divmod(np.arange(n, dtype=np.int64), n_a)
    kind, c, gu, gw = world_kind(i + ia, j + jb)
    per = np.where(rng.random(n) < fill, rng.integers(1, most + 1, n), 0)
    cell = np.repeat(np.arange(n, dtype=np.int64), per)
    m = len(cell)
    u = 2 * rng.integers(0, sub, m) - (sub - 1)
    w = 2 * rng.integers(0, sub, m) - (sub - 1)
    kd = kind[cell]
    u = np.where(kd == 4, 2 * ((i[cell] + ia + rng.integers(0, 3)) % sub) - (sub - 1), u)      # a sliver: one column a frame
    noise = np.where(kd == 1, rng.integers(-3, 4, m), np.where(kd == 3, rng.integers(-60, 61, m), 0))
    k = c[cell] + gu[cell] * u + gw[cell] * w + noise
    return cell, k, u, w


def frame_tables(rng, n_a, n_b, ia, jb, **kw):
    """-> (count, sum, sum2, moments) as a slope call of `sub` would have written them for frame_points' points."""
    return sums_of(n_a * n_b, *frame_points(rng, n_a, n_b, ia, jb, **kw))


def strip(u, slope_u=3, slope_w=2, base=100):
    """The issue's example: the strip u of one cell, w = -7 .. 7 odd, k = base + slope_u u + slope_w w."""
    w = np.arange(-7, 8, 2)
    us = np.full(8, u)
    return np.zeros(8, dtype=np.int64), base + slope_u * us + slope_w * w, us, w
