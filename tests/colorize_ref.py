"""Restatement of colorizeDepth (reference src/depth_map_fusion.cpp:306-360), the spec d2pc_colorize_table is pinned
to, and a plain-Python model of the depth_map_fusion node's state (class RefNode).

Per 8-bit pixel g:
  d  = (unsigned char)(40 + 0.8 g)             in double            (= 40 + 4 g // 5)
  H  = 255 - (255 - d) * 280 // 255            integers, 19 .. 243
  hi = (H // 60) % 6                           0 .. 4
  f  = H / 60.f - float(H // 60)               IEEE float32, every operation rounded to float32
  p = 0, q = 1 - f, t = 1 - (1 - f), V = 1
  (x, y, z) = hi: 0 (p,t,V)  1 (p,V,q)  2 (t,V,p)  3 (V,q,p)  4 (V,p,t)
  bytes in memory order = trunc(clamp(x) * 255.f), trunc(clamp(y) * 255.f), trunc(clamp(z) * 255.f)
  d == 40 (g = 0 and g = 1)  ->  (0, 0, 0)

The vectorised table below keeps every intermediate in np.float32 arrays; tests/golden/make_colorize_golden.py
derives the same table entry by entry with scalars."""
import numpy as np

import oracle
import score_filter_ref

F32 = np.float32


def depth_d(g=None):
    """Step 1 in double, as written: (unsigned char)(40 + 0.8 * g)."""
    g = np.arange(256, dtype=np.float64) if g is None else np.asarray(g, dtype=np.float64)
    return np.floor(40.0 + 0.8 * g).astype(np.int64)


def hue(d):
    d = np.asarray(d, dtype=np.int64)
    H = 255 - (255 - d) * 280 // 255
    return H, (H // 60) % 6


def colorize_table(f_dtype=np.float32, divide=True):
    """The 256 x 3 table.  f_dtype = np.float64 evaluates the whole float chain in double (excess precision,
    FLT_EVAL_METHOD != 0); divide=False replaces H / 60.f by H * (1 / 60.f): the variants the table must differ from."""
    d = depth_d()
    H, hi = hue(d)
    Hf = H.astype(F32)
    if divide:
        quo = (Hf.astype(f_dtype) / f_dtype(F32(60.0))).astype(f_dtype)
    else:
        quo = (Hf * (F32(1.0) / F32(60.0))).astype(F32)
    f = (quo - (H // 60).astype(f_dtype)).astype(f_dtype)
    one, zero = f_dtype(1.0), f_dtype(0.0)
    q = (one - f).astype(f_dtype)
    t = (one - (one - f).astype(f_dtype)).astype(f_dtype)
    p = np.full(256, zero, dtype=f_dtype)
    V = np.full(256, one, dtype=f_dtype)
    pick = {0: (p, t, V), 1: (p, V, q), 2: (t, V, p), 3: (V, q, p), 4: (V, p, t), 5: (q, p, V)}
    out = np.zeros((256, 3), dtype=np.uint8)
    for k, trio in pick.items():
        sel = hi == k
        for c in range(3):
            v = np.maximum(zero, np.minimum(trio[c], one)).astype(f_dtype)
            out[sel, c] = np.trunc((v * f_dtype(255.0)).astype(f_dtype))[sel].astype(np.uint8)
    out[d == 40] = 0
    return out


_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = colorize_table()
    return _TABLE


def colorize(gray):
    """(..., H, W) uint8 -> (..., H, W, 3) uint8."""
    assert gray.dtype == np.uint8
    return table()[gray]


def colorize_view(frame, view=None, rotate_cw=False):
    """What d2pc_colorize_device computes for one frame: (rgb, gray) of the view of the (rotated) frame."""
    img = oracle.rotate_cw(np.ascontiguousarray(frame)) if rotate_cw else frame
    if view is not None:
        x, y, w, h = view
        img = img[y:y + h, x:x + w]
    return colorize(img), img.copy()


class RefNode:
    """The depth_map_fusion node as a sequence of statements on numpy arrays standing for its cv::Mat members.  As in
    the reference, score and grad of a camera are ONE array object (:77,:96) and cropped_score_combined_ is the very
    array of camera 1's score (:113), so a fusion overwrites it in place."""

    CROP = (0, 40, 30, 10)

    def __init__(self, cols, rows, offset_x=0, offset_y=0, rule=oracle.FUSE_GRAD_FILTER, form=4):
        self.cols, self.rows, self.ox, self.oy, self.rule, self.form = cols, rows, offset_x, offset_y, rule, form
        # The frame the reference fuses INTO is cropToSquare(image) of the incoming message (:106): arguments 0, side
        # min(cols, rows) - |offset_y_| (:253).  The loop (:115-123) covers min(cols, rows) - max(|offset_x|, |offset_y|)
        # of it.  Only with |offset_x| <= |offset_y| are the two the same square, as _fuse() below takes them to be;
        # beyond that the compiled reference publishes a larger fused map (200 x 140 with 9 / -6: 94 x 94, not 91 x 91)
        # with a margin of raw camera-2 pixels, which neither this model nor the product reproduces
        # (tests/README_reference.md).
        assert abs(offset_x) <= abs(offset_y), "|offset_x| > |offset_y|: refused by the product, not modelled here"
        self.sq1 = oracle.crop_to_square(cols, rows, offset_x, offset_y)
        self.sq2 = oracle.crop_to_square(rows, cols, -offset_x, -offset_y, offset_y)  # member offset_y_ (:253)
        assert self.sq1[2] == self.sq2[2]
        self.n = self.sq1[2]
        self.depth_1 = self.depth_2 = None
        self.score_1 = self.score_1_grad = self.score_2 = self.score_2_grad = self.combined = None

    @staticmethod
    def _view(img, sq):
        x, y, n = sq
        return img[y:y + n, x:x + n]

    def disparity_1(self, frame):
        self.depth_1 = self._view(frame, self.sq1).copy()
        return {"cropped_depth_1": colorize(self.depth_1)}

    def disparity_2(self, frame):
        self.depth_2 = self._view(oracle.rotate_cw(np.ascontiguousarray(frame)), self.sq2).copy()
        out = {"cropped_depth_2": colorize(self.depth_2)}
        out.update(self._fuse())
        return out

    def matching_score_1(self, frame):
        out, _ = score_filter_ref.score_filter(frame, self.sq1, 0, self.form)  # out = min(255, score + 2 B)
        self.score_1_grad = out
        self.score_1 = self.score_1_grad  # one buffer (:77)
        return {"cropped_score_1": self.score_1.copy()}

    def matching_score_2(self, frame):
        out, _ = score_filter_ref.score_filter(oracle.rotate_cw(np.ascontiguousarray(frame)), self.sq2, 1, self.form)
        self.score_2_grad = out
        self.score_2 = self.score_2_grad  # (:96)
        return {"cropped_score_2": self.score_2.copy()}

    def _fuse(self):
        if self.depth_1 is None or self.depth_2 is None or self.score_1 is None or self.score_2 is None:
            return {}  # (:106-109)
        self.combined = self.score_1  # the same buffer (:113)
        planes = [np.ascontiguousarray(p) for p in (self.depth_1, self.depth_2, self.score_1, self.score_2,
                                                    self.score_1_grad, self.score_2_grad)]
        fused, comb = oracle.fuse(planes, rule=self.rule, crop=self.CROP)
        self.combined[...] = comb  # ... written in place: score_1 and score_1_grad now hold min(grad1, grad2)
        assert self.score_1 is self.combined and self.score_1_grad is self.combined
        return {"combined_score": self.combined.copy(), "gradient": colorize(fused), "fused_depth_map": fused}
