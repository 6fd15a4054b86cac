"""Integer restatement of the matching-score pre-filter of MatchingScoreCb1/2 (reference
src/depth_map_fusion.cpp:64-99), the spec d2pc_score_filter_device is pinned to.

  A   = rint_even(G13 of the frame round the square / 65536)     reflect101 about the FRAME (the square is a view)
  M   = 255 * (I >= 1017),  I = sum d * sum s * A                 reflect101 about the square
  B   = CV4: (255 * G21(M/255) + 32768) >> 16,  CV3: rint_even(255 * G21(M/255) / 65536)
  out = min(255, S + 2 B)

The tap tables are derived here in fp64 from the Gaussian formula and OpenCV's rounding rules, never typed in."""
import math

import numpy as np

SOBEL_S = np.array([1, 6, 15, 20, 15, 6, 1], np.int64)    # getSobelKernels(ksize 7, order 0)
SOBEL_D = np.array([1, 2, -1, -4, -1, 2, 1], np.int64)    # ... order 2
THRESHOLD_I = 1017                                        # round(0.03 I) > 30  <=>  I >= 1017 (test_score_filter_cpu)


def gauss_bitexact(n, sigma):
    """OpenCV 4.x getGaussianKernelBitExact (fp64 in place of softdouble): exp(-(x/2)^2 / (2 sigma^2)) over x = 1-n,
    3-n, ..., normalised to sum 1 with the centre tap 1 * (1 / sum)."""
    scale2 = -0.125 / (sigma * sigma)
    half = [math.exp(float(x * x) * scale2) for x in range(1 - n, 0, 2)]
    mul = 1.0 / (sum(half) * 2 + 1.0)
    h = [v * mul for v in half]
    return h + [mul] + h[::-1]


def gauss_cv3(n, sigma):
    """OpenCV 3.2 getGaussianKernel(n, sigma, CV_32F): float taps, double sum, float(tap * (1 / sum))."""
    scale2 = -0.5 / (sigma * sigma)
    cf = [np.float32(math.exp(scale2 * (i - (n - 1) * 0.5) ** 2)) for i in range(n)]
    inv = 1.0 / sum(float(c) for c in cf)
    return [float(np.float32(float(c) * inv)) for c in cf]


def general_taps(g):
    """The general 8-bit sepFilter2D path: convertTo(CV_32S, 256) = cvRound(float(g) * 256) (half to even).
    Returns (taps, margins): margin = distance of float(g) * 256 from the nearest rounding boundary (in 1/256)."""
    v = [float(np.float32(x)) * 256.0 for x in g]
    taps = [int(np.rint(x)) for x in v]
    margins = [abs(abs(x - math.floor(x)) - 0.5) for x in v]
    return np.array(taps, np.int64), np.array(margins)


def fixed_point_taps(g, bits=8):
    """OpenCV 4.x getGaussianKernelFixedPoint_ED: error-diffused cvRound from the outside in, the centre takes the
    remainder (taps sum to 1 << bits).  Margins as in general_taps (the centre has none)."""
    n = len(g)
    t, m = [0] * n, [math.inf] * n
    err, s = 0.0, 0
    for i in range(n // 2):
        adj = g[i] * (1 << bits) + err
        v = int(np.rint(adj))
        m[i] = m[n - 1 - i] = abs(abs(adj - math.floor(adj)) - 0.5)
        err = adj - v
        t[i] = t[n - 1 - i] = v
        s += v
    t[n // 2] = (1 << bits) - 2 * s
    return np.array(t, np.int64), np.array(m)


def tap_tables(form=4):
    """(t13, t21) of a form: 4 = OpenCV 4.x, 3 = OpenCV 3.2.  G13 takes the general path in both (a view)."""
    t13, _ = general_taps(gauss_bitexact(13, 3.0))
    if form == 4:
        t21, _ = fixed_point_taps(gauss_bitexact(21, 10.0))
    elif form == 3:
        t21, _ = general_taps(gauss_cv3(21, 10.0))
    else:
        raise ValueError(form)
    return t13, t21


def refl(idx, length):
    """cv::borderInterpolate(BORDER_REFLECT_101), vectorised: the mirror-periodic extension."""
    idx = np.asarray(idx, np.int64)
    if length == 1:
        return np.zeros_like(idx)
    per = 2 * (length - 1)
    p = np.mod(idx, per)
    return np.where(p < length, p, per - p)


def rint_even_16(s):
    """rint_even(s / 65536) for integer s >= 0."""
    s = np.asarray(s, np.int64)
    q, r = s >> 16, s & 0xFFFF
    return q + ((r > 0x8000) | ((r == 0x8000) & ((q & 1) == 1)))


def _sep(img, kr, kc):
    """sum_v kc[v] * sum_u kr[u] * img[v + i, u + j] for an image padded by the kernels' radii."""
    rr, rc = len(kr) // 2, len(kc) // 2
    h, w = img.shape[0] - 2 * rc, img.shape[1] - 2 * rr
    rows = sum(int(kr[u]) * img[:, u:u + w] for u in range(len(kr)))
    return sum(int(kc[v]) * rows[v:v + h, :] for v in range(len(kc)))


def _pad_sq(img, r):
    n = img.shape[0]
    i = refl(np.arange(-r, n + r), n)
    return img[np.ix_(i, i)]


def stages(frame, square, direction, form=4):
    """All stages of one frame: dict with A, I, M (0/1), B, out (n x n each)."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 2
    x, y, n = square
    h, w = frame.shape
    t13, t21 = tap_tables(form)
    rows = refl(y + np.arange(-6, n + 6), h)
    cols = refl(x + np.arange(-6, n + 6), w)
    a = rint_even_16(_sep(frame[np.ix_(rows, cols)].astype(np.int64), t13, t13))
    kr, kc = (SOBEL_S, SOBEL_D) if direction == 0 else (SOBEL_D, SOBEL_S)
    i = _sep(_pad_sq(a, 3), kr, kc)
    m = (i >= THRESHOLD_I).astype(np.int64)
    v = 255 * _sep(_pad_sq(m, 10), t21, t21)
    b = (v + 0x8000) >> 16 if form == 4 else rint_even_16(v)
    s = frame[y:y + n, x:x + n].astype(np.int64)
    out = np.minimum(255, s + 2 * b)
    return {"A": a, "I": i, "M": m, "B": b, "out": out}


def score_filter(frame, square, direction, form=4):
    """(out, grad) as uint8 n x n: what d2pc_score_filter_device writes."""
    st = stages(frame, square, direction, form)
    return st["out"].astype(np.uint8), st["B"].astype(np.uint8)
