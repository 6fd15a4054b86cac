"""The three OpenCV filters the compiled reference (oracle/ref.py) reaches through hooks, built from the stages of
score_filter_ref -- this project's reading of OpenCV, NOT pinned by the reference.  What the reference pins is
everything around them: which filter runs when, on which Mat, with which dx / dy, in place or not, and what happens
to the result (score + 2 grad, the shared buffers).

  GaussianBlur 13 x 13, sigma 3   general 8-bit path: taps * 256 rounded, rint_even(sum / 65536); BORDER_REFLECT_101
                                  about the PARENT of a view (OpenCV reads a view's surroundings)
  Sobel ksize 7, scale 0.03       saturate(rint_even(0.03 * I)), I = the integer separable response; reflect-101
                                  about the Mat itself (it is no view there)
  threshold type 0 (BINARY)       src > thresh ? maxval : 0
  GaussianBlur 21 x 21, sigma 10  form 4: fixed-point taps, (sum + 32768) >> 16; form 3: general path; about the Mat
"""
import numpy as np

import score_filter_ref as sf
from oracle import ref


def _reflected(view, radius):
    """The view's pixels with `radius` more on every side, reflect-101 about the allocation it lies in."""
    parent = view.parent_array()
    rows = sf.refl(view.y + np.arange(-radius, view.rows + radius), view.parent_rows)
    cols = sf.refl(view.x + np.arange(-radius, view.cols + radius), view.parent_cols)
    return parent[np.ix_(rows, cols)].astype(np.int64)


def make_hooks(form=4, log=None):
    """-> (gaussian, sobel, threshold) for ref.set_hooks.  `log`, a list, receives one tuple per call."""
    t13, t21 = sf.tap_tables(form)

    def gaussian(src, dst, kx, ky, sigma):
        assert kx == ky and (kx, sigma) in ((13, 3.0), (21, 10.0)), (kx, ky, sigma)
        if log is not None:
            log.append(("gaussian", kx, sigma, (src.x, src.y, src.cols, src.rows), (src.parent_cols, src.parent_rows),
                        src.data == dst.data))
        if kx == 13:
            out = sf.rint_even_16(sf._sep(_reflected(src, 6), t13, t13))
        else:
            v = sf._sep(_reflected(src, 10), t21, t21)
            out = (v + 0x8000) >> 16 if form == 4 else sf.rint_even_16(v)
        assert out.min() >= 0 and out.max() <= 255
        dst.array()[...] = out.astype(np.uint8)

    def sobel(src, dst, dx, dy, ksize, scale):
        assert ksize == 7 and scale == 0.03 and (dx, dy) in ((0, 2), (2, 0)), (dx, dy, ksize, scale)
        if log is not None:
            log.append(("sobel", dx, dy, (src.x, src.y, src.cols, src.rows), (src.parent_cols, src.parent_rows),
                        src.data == dst.data))
        kr = sf.SOBEL_D if dx == 2 else sf.SOBEL_S   # along a row: the x derivative's order
        kc = sf.SOBEL_D if dy == 2 else sf.SOBEL_S
        i = sf._sep(_reflected(src, 3), kr, kc)
        dst.array()[...] = np.clip(np.rint(scale * i.astype(np.float64)), 0, 255).astype(np.uint8)

    def threshold(src, dst, thresh, maxval, kind):
        assert kind == 0, kind
        if log is not None:
            log.append(("threshold", thresh, maxval, kind, src.data == dst.data))
        dst.array()[...] = np.where(src.array().astype(np.float64) > thresh, np.uint8(maxval), np.uint8(0))

    return gaussian, sobel, threshold


def install(form=4, log=None):
    ref.set_hooks(*make_hooks(form, log))
