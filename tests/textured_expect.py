"""Expected bytes of a textured cloud (d2pc_texture_device), in numpy and independent of the library: a record is the
producer's own 16 bytes, then the texture word gathered at the point's source pixel, then three zero words.  Everything
is uint32 bit patterns, so NaN payloads and -0.0 compare exactly."""
import numpy as np

POINT_XYZI, POINT_XYZRGB = 1, 2
TEX_U8, TEX_U16, TEX_F32, TEX_RGB8, TEX_BGR8, TEX_MONO8 = range(1, 7)
FORMATS = {"u8": (POINT_XYZI, TEX_U8), "u16": (POINT_XYZI, TEX_U16), "f32": (POINT_XYZI, TEX_F32),
           "rgb8": (POINT_XYZRGB, TEX_RGB8), "bgr8": (POINT_XYZRGB, TEX_BGR8), "mono8": (POINT_XYZRGB, TEX_MONO8)}
BYTES_PER_PIXEL = {"u8": 1, "u16": 2, "f32": 4, "rgb8": 3, "bgr8": 3, "mono8": 1}


def roi_pixels(h, w, border):
    """Frame-local pixel index v * w + u of the PARITY layout's position i, row-major over the inset ROI."""
    v, u = np.mgrid[border:h - border, border:w - border]
    return (v * w + u).reshape(-1).astype(np.uint32)


def plane_words(planes, fmt):
    """The texture word of every pixel: planes (F, H, W) -- rgb8 / bgr8: (F, H, W, 3) uint8 -- -> (F * H * W,) uint32."""
    p = np.asarray(planes)
    if fmt in ("u8", "u16"):
        assert p.dtype == (np.uint8 if fmt == "u8" else np.uint16)
        return p.astype(np.float32).view(np.uint32).reshape(-1)   # exact: every 16-bit integer is a float32
    if fmt == "f32":
        assert p.dtype == np.float32
        return np.ascontiguousarray(p).view(np.uint32).reshape(-1)  # a bit copy, NaN payloads included
    assert p.dtype == np.uint8
    if fmt == "mono8":
        r = g = b = p.astype(np.uint32)
    else:
        c = p.astype(np.uint32)
        r, g, b = (c[..., 0], c[..., 1], c[..., 2]) if fmt == "rgb8" else (c[..., 2], c[..., 1], c[..., 0])
    return (np.uint32(255 << 24) | (r << 16) | (g << 8) | b).astype(np.uint32).reshape(-1)


def expect_records(points, pix, planes, fmt, frame=None, n_declared=None):
    """points: (n, 4) float32 or uint32, the producer's records; pix: (n,) their source pixel indices.
    frame=None: the merged layout (pix = f * W * H + v * W + u over the declared frames); frame=f: frame-local indices
    of frame f.  n_declared: frames the descriptor declares (default all of `planes`); a pixel index at or beyond the
    declared pixels gives word 0.  -> (n, 8) uint32."""
    p = np.asarray(planes)
    f, h, w = p.shape[:3]
    n_declared = f if n_declared is None else n_declared
    words = plane_words(p, fmt)
    pix = np.asarray(pix).astype(np.int64)
    if frame is None:
        ok, src = pix < n_declared * h * w, pix
    else:
        ok, src = pix < h * w, frame * h * w + pix
    pts = np.ascontiguousarray(points)
    pts = pts.view(np.uint32) if pts.dtype == np.float32 else pts.astype(np.uint32)
    out = np.zeros((len(pix), 8), dtype=np.uint32)
    out[:, :4] = pts.reshape(-1, 4)
    out[:, 4] = np.where(ok, words[np.where(ok, src, 0)], 0)
    return out
