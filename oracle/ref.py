"""The reference's own depth_map_fusion.cpp as a checker: oracle/_ref/libref_fusion.so is the reference's unmodified
.cpp and .hpp compiled against the stand-in headers of oracle/ref_shim/ (our cv::Mat, ros::NodeHandle, cv_bridge)
plus the C-ABI harness ref_harness.cpp.  TEST INFRASTRUCTURE ONLY; the product never imports it.

What comes out of it is the reference's arithmetic: the nine rules, getFusedDistance, cropToSquare / cropMat /
rotateMat, colorizeDepth, the aliasing of its cv::Mat members and the publishing order.  cv::GaussianBlur, cv::Sobel
and cv::threshold are hooks (set_hooks): their arithmetic stays this project's reading of OpenCV (tests/ref_filters.py),
as does cv::medianBlur's, which the stand-in implements as a plain order statistic.

The reference's sources are never copied: build_ref() compiles them where they lie (D2PC_REFERENCE_DIR) into
oracle/_ref/, which git ignores.  Where that directory does not exist, build_ref() does nothing and a library built
earlier keeps serving."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(_HERE, "ref_shim")
REF_DIR_OUT = os.path.join(_HERE, "_ref")
LIB_PATH = os.path.join(REF_DIR_OUT, "libref_fusion.so")
CXXFLAGS = ["-std=c++14", "-O1", "-fPIC", "-shared", "-fno-access-control", "-ffp-contract=off"]

OK, THREW, NO_HOOK, BAD_ARG = range(4)
DISPARITY_1, DISPARITY_2, MATCHING_SCORE_1, MATCHING_SCORE_2 = range(4)
CALLS = {"D1": DISPARITY_1, "D2": DISPARITY_2, "S1": MATCHING_SCORE_1, "S2": MATCHING_SCORE_2}


def reference_dir() -> str:
    return os.environ.get("D2PC_REFERENCE_DIR", "/root/reference")


def reference_sources():
    """(the .cpp, the include directory) of the reference, or None where it is not on this machine."""
    root = reference_dir()
    cpp = os.path.join(root, "src", "depth_map_fusion.cpp")
    inc = os.path.join(root, "include")
    if os.path.isfile(cpp) and os.path.isfile(os.path.join(inc, "disparity_to_point_cloud", "depth_map_fusion.hpp")):
        return cpp, inc
    return None


def shim_files():
    out = []
    for d, _, names in os.walk(SHIM):
        out += [os.path.join(d, n) for n in names]
    return sorted(out)


def build_ref(force: bool = False):
    """Compile the reference + harness.  No reference directory: a no-op.  A failing compile raises."""
    src = reference_sources()
    if src is None:
        return LIB_PATH if os.path.exists(LIB_PATH) else None
    cpp, inc = src
    deps = shim_files() + [cpp, os.path.join(inc, "disparity_to_point_cloud", "depth_map_fusion.hpp"), os.path.abspath(__file__)]
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(f) <= os.path.getmtime(LIB_PATH) for f in deps):
        return LIB_PATH
    os.makedirs(REF_DIR_OUT, exist_ok=True)
    tmp = LIB_PATH + ".tmp%d" % os.getpid()
    cmd = [os.environ.get("CXX", "g++")] + CXXFLAGS + ["-I", SHIM, "-I", inc, "-o", tmp, cpp, os.path.join(SHIM, "ref_harness.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError("compiling the reference against oracle/ref_shim failed:\n%s\n%s" % (" ".join(cmd), p.stderr[-4000:]))
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


def available() -> bool:
    return os.path.exists(LIB_PATH)


class View(ctypes.Structure):
    """ref_view of ref_shim/opencv2/imgproc/imgproc.hpp."""
    _fields_ = [("data", ctypes.c_void_p), ("step", ctypes.c_ulonglong), ("rows", ctypes.c_int), ("cols", ctypes.c_int),
                ("parent", ctypes.c_void_p), ("parent_rows", ctypes.c_int), ("parent_cols", ctypes.c_int),
                ("x", ctypes.c_int), ("y", ctypes.c_int)]

    def array(self):
        """The view's pixels as a numpy array over the reference's own memory (writable)."""
        buf = (ctypes.c_ubyte * (self.step * (self.rows - 1) + self.cols)).from_address(self.data)
        return np.lib.stride_tricks.as_strided(np.frombuffer(buf, dtype=np.uint8), (self.rows, self.cols), (self.step, 1))

    def parent_array(self):
        buf = (ctypes.c_ubyte * (self.step * (self.parent_rows - 1) + self.parent_cols)).from_address(self.parent)
        return np.lib.stride_tricks.as_strided(np.frombuffer(buf, dtype=np.uint8), (self.parent_rows, self.parent_cols),
                                               (self.step, 1))


class Topic(ctypes.Structure):
    _fields_ = [("topic", ctypes.c_char_p), ("encoding", ctypes.c_char_p), ("frame_id", ctypes.c_char_p),
                ("seq", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("step", ctypes.c_uint32),
                ("data", ctypes.c_void_p), ("bytes", ctypes.c_size_t)]


_VP = ctypes.POINTER(View)
GAUSSIAN_HOOK = ctypes.CFUNCTYPE(ctypes.c_int, _VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_double)
SOBEL_HOOK = ctypes.CFUNCTYPE(ctypes.c_int, _VP, _VP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double)
THRESHOLD_HOOK = ctypes.CFUNCTYPE(ctypes.c_int, _VP, _VP, ctypes.c_double, ctypes.c_double, ctypes.c_int)

_lib = None
_hooks = None  # keeps the installed callbacks alive


def lib():
    global _lib
    if _lib is None:
        if not available():
            raise RuntimeError("oracle/_ref/libref_fusion.so is not built (oracle.build() builds it where the reference is present)")
        L = ctypes.CDLL(LIB_PATH)
        ip, u8p = ctypes.POINTER(ctypes.c_int), ctypes.c_void_p
        L.ref_last_error.restype = ctypes.c_char_p
        L.ref_set_hooks.argtypes = [GAUSSIAN_HOOK, SOBEL_HOOK, THRESHOLD_HOOK]
        L.ref_set_hooks.restype = None
        L.ref_fuse_pixels.argtypes = [ctypes.c_int, ctypes.c_size_t] + [u8p] * 6 + [ctypes.c_void_p]
        L.ref_crop_to_square.argtypes = [ctypes.c_int] * 5 + [ip]
        L.ref_crop_mat.argtypes = [ctypes.c_int] * 6 + [ip]
        L.ref_rotate_mat.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, u8p, ip]
        L.ref_colorize.argtypes = [u8p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, u8p]
        L.ref_geometry.argtypes = [ctypes.c_int] * 4 + [ip]
        L.ref_geometry_batch.argtypes = [ctypes.c_size_t] + [ctypes.c_void_p] * 6
        L.ref_node_create.argtypes = [ctypes.c_int] * 4
        L.ref_node_create.restype = ctypes.c_void_p
        L.ref_node_destroy.argtypes = [ctypes.c_void_p]
        L.ref_node_destroy.restype = None
        L.ref_node_offsets.argtypes = [ctypes.c_void_p, ip]
        L.ref_node_callback.argtypes = [ctypes.c_void_p, ctypes.c_int, u8p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_uint32, ctypes.c_char_p]
        L.ref_node_published.argtypes = [ctypes.c_void_p]
        L.ref_node_topic.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(Topic)]
        _lib = L
    return _lib


class RefThrew(Exception):
    """The reference threw (a cv::Exception where OpenCV's CV_Assert would)."""


class RefNoHook(Exception):
    """A filter was reached with no hook installed."""


def _check(st):
    if st == THREW:
        raise RefThrew(lib().ref_last_error().decode())
    if st == NO_HOOK:
        raise RefNoHook(lib().ref_last_error().decode())
    if st != OK:
        raise ValueError("bad argument (%d)" % st)


def set_hooks(gaussian=None, sobel=None, threshold=None):
    """Install Python callables (View src, View dst, ...) -> None as the three filters; None uninstalls."""
    global _hooks

    def wrap(proto, fn):
        if fn is None:
            return proto()

        def call(src, dst, *args):
            try:
                fn(src.contents, dst.contents, *args)
                return 0
            except Exception:  # an exception must not cross the C frames
                import traceback
                traceback.print_exc()
                return 1
        return proto(call)

    hooks = (wrap(GAUSSIAN_HOOK, gaussian), wrap(SOBEL_HOOK, sobel), wrap(THRESHOLD_HOOK, threshold))
    lib().ref_set_hooks(*hooks)
    _hooks = hooks


def fuse_pixels(rule, d1, d2, s1, s2, g1=None, g2=None) -> np.ndarray:
    """Rule 0..8 on flat uint8 arrays -> int16; -1 marks weightedAverage's division by zero (not evaluated)."""
    arrs = [np.ascontiguousarray(a, dtype=np.uint8).ravel() for a in (d1, d2, s1, s2)]
    n = arrs[0].size
    assert all(a.size == n for a in arrs)
    gs = [None if g is None else np.ascontiguousarray(g, dtype=np.uint8).ravel() for g in (g1, g2)]
    out = np.empty(n, dtype=np.int16)
    _check(lib().ref_fuse_pixels(rule, n, *[a.ctypes.data for a in arrs], *[None if g is None else g.ctypes.data for g in gs],
                                 out.ctypes.data))
    return out


def crop_to_square(cols, rows, offset_x=0, offset_y=0, member_offset_y=None):
    """-> (x, y, w, h) of the view cropToSquare returns; raises RefThrew."""
    r = (ctypes.c_int * 4)()
    _check(lib().ref_crop_to_square(cols, rows, offset_x, offset_y, offset_y if member_offset_y is None else member_offset_y, r))
    return tuple(r)


def crop_mat(cols, rows, left, right, top, bottom):
    r = (ctypes.c_int * 4)()
    _check(lib().ref_crop_mat(cols, rows, left, right, top, bottom, r))
    return tuple(r)


def rotate_mat(img: np.ndarray) -> np.ndarray:
    assert img.dtype == np.uint8 and img.ndim == 2 and img.strides[1] == 1
    rows, cols = img.shape
    out = np.empty(rows * cols, dtype=np.uint8)
    size = (ctypes.c_int * 2)()
    _check(lib().ref_rotate_mat(img.ctypes.data, img.strides[0], cols, rows, out.ctypes.data, size))
    return out.reshape(size[1], size[0])


def colorize(gray: np.ndarray, as_view=False) -> np.ndarray:
    assert gray.dtype == np.uint8 and gray.ndim == 2 and gray.strides[1] == 1
    rows, cols = gray.shape
    out = np.empty((rows, cols, 3), dtype=np.uint8)
    _check(lib().ref_colorize(gray.ctypes.data, gray.strides[0], cols, rows, int(as_view), out.ctypes.data))
    return out


def geometry_batch(cols, rows, offset_x, offset_y):
    """Flat int arrays -> (out (N, 16), threw (N,)): sq1, sq2, the fuse image's square, the fused map (x, y, w, h
    each); threw has bit 1 / 2 / 4 / 8 set where that stage of the reference threw."""
    a = [np.ascontiguousarray(v, dtype=np.int32).ravel() for v in (cols, rows, offset_x, offset_y)]
    n = a[0].size
    out = np.zeros((n, 16), dtype=np.int32)
    status = np.zeros(n, dtype=np.int32)
    lib().ref_geometry_batch(n, *[v.ctypes.data for v in a], out.ctypes.data, status.ctypes.data)
    return out, status


class Node:
    """One DepthMapFusion of the reference.  callback() -> [(topic, encoding, width, height, step, bytes)] in
    publishing order."""

    def __init__(self, offset_x=None, offset_y=None):
        self._h = lib().ref_node_create(offset_x or 0, offset_y or 0, offset_x is not None, offset_y is not None)
        self.warnings = lib().ref_node_warnings()
        self._seq = 0

    def close(self):
        if self._h:
            lib().ref_node_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def offsets(self):
        o = (ctypes.c_int * 2)()
        lib().ref_node_offsets(self._h, o)
        return tuple(o)

    def callback(self, which, frame: np.ndarray):
        which = CALLS.get(which, which)
        assert frame.dtype == np.uint8 and frame.ndim == 2 and frame.strides[1] == 1
        self._seq += 1
        st = lib().ref_node_callback(self._h, which, frame.ctypes.data, frame.strides[0], frame.shape[1], frame.shape[0],
                                     self._seq, b"cam")
        _check(st)
        out = []
        t = Topic()
        for i in range(lib().ref_node_published(self._h)):
            lib().ref_node_topic(self._h, i, ctypes.byref(t))
            out.append((t.topic.decode(), t.encoding.decode(), t.width, t.height, t.step, ctypes.string_at(t.data, t.bytes)))
        return out
