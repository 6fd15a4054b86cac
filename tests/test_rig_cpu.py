"""The rig session of the C ABI (d2pc_rig_*, include/d2pc.h) where no device is needed: struct layouts, the host
arithmetic of d2pc_rig_geometry and its refusals, d2pc_rig_compose_q bit for bit, the exported symbols."""
import ctypes
import subprocess

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
from disparity_to_point_cloud_amd import capi

INVALID_ARG, BAD_DTYPE, BAD_SIZE = 1, 2, 3
RIG_SYMBOLS = ("d2pc_rig_config_init", "d2pc_rig_geometry", "d2pc_rig_compose_q", "d2pc_rig_create", "d2pc_rig_set_q",
               "d2pc_rig_get_q", "d2pc_rig_process_device", "d2pc_rig_destroy")
COMPACT_TILE = 1024   # ROI pixels per tile of the COMPACT kernels: the session holds 16 bytes per tile at border 0
TABLE_ENTRY = 184     # bytes of one camera's calibration on the device


def test_struct_sizes_and_defaults():
    assert ctypes.sizeof(capi.RigConfig) == 32
    assert ctypes.sizeof(capi.RigGeometry) == 3 * ctypes.sizeof(ctypes.c_size_t) + 16
    cfg = capi.RigConfig()
    cfg.width = cfg.height = cfg.n_cameras = 99
    cfg.reserved[2] = 7
    d2pc.load_library().d2pc_rig_config_init(ctypes.byref(cfg))
    assert (cfg.struct_size, cfg.n_cameras, cfg.width, cfg.height, cfg.dtype) == (32, 1, 0, 0, d2pc.DTYPE_F32)
    assert list(cfg.reserved) == [0, 0, 0]
    assert capi.RIG_MAX_CAMERAS == 64
    d2pc.load_library().d2pc_rig_config_init(None)   # a null pointer is ignored


@pytest.mark.parametrize("n,w,h,border,dtype", [
    (1, 752, 480, 40, d2pc.DTYPE_U8), (3, 70, 37, 3, d2pc.DTYPE_F32), (5, 20, 12, 2, d2pc.DTYPE_U16),
    (64, 3840, 2160, 0, d2pc.DTYPE_F32), (16, 16384, 16384, 1, d2pc.DTYPE_U8), (9, 300, 260, 2, d2pc.DTYPE_F32),
])
def test_geometry_is_plain_integer_arithmetic(n, w, h, border, dtype):
    g = d2pc.rig_geometry(d2pc.rig_config_init(n_cameras=n, width=w, height=h, dtype=dtype), border)
    roi = max(w - 2 * border, 0) * max(h - 2 * border, 0)
    assert g.roi_points == roi == d2pc.roi_points(w, h, border)
    assert g.capacity_points == n * roi
    assert g.device_bytes == n * TABLE_ENTRY + n * -(-(w * h) // COMPACT_TILE) * 16
    assert g.index_available == int(n * w * h <= 2**32)
    assert list(g.reserved) == [0, 0, 0]


def test_geometry_refusals():
    L = d2pc.load_library()
    out = capi.RigGeometry()

    def status(border=2, **kw):
        cfg = d2pc.rig_config_init(**dict(dict(n_cameras=3, width=70, height=37), **kw))
        return L.d2pc_rig_geometry(ctypes.byref(cfg), border, ctypes.byref(out))

    assert status() == 0
    assert status(n_cameras=0) == INVALID_ARG and status(n_cameras=65) == INVALID_ARG and status(n_cameras=64) == 0
    assert status(dtype=3) == BAD_DTYPE and status(dtype=-1) == BAD_DTYPE      # (MONO16 is a host-entry dtype)
    assert status(width=0) == BAD_SIZE and status(height=0) == BAD_SIZE and status(width=-5) == BAD_SIZE
    assert status(border=-1) == INVALID_ARG and status(border=16385) == INVALID_ARG
    assert status(struct_size=28) == INVALID_ARG
    assert L.d2pc_rig_geometry(None, 0, ctypes.byref(out)) == INVALID_ARG
    assert L.d2pc_rig_geometry(ctypes.byref(d2pc.rig_config_init(width=8, height=8)), 0, None) == INVALID_ARG
    # a point's position in the merged cloud is 32 bits: n * roi_n >= 2^32 is refused, one point fewer is not
    assert status(n_cameras=16, width=16384, height=16384, border=0) == BAD_SIZE          # = 2^32
    assert status(n_cameras=16, width=16384, height=16384, border=1) == 0
    assert out.capacity_points == 16 * 16382 * 16382 < 2**32 and out.index_available == 1    # n W H = 2^32 exactly
    assert status(n_cameras=64, width=16384, height=16384, border=0) == BAD_SIZE
    assert status(n_cameras=1, width=65536, height=32769, border=0) == BAD_SIZE            # a frame beyond 2^31 pixels
    # the index holds f W H + v W + u: unavailable once the batch has more than 2^32 pixels
    assert status(n_cameras=16, width=16386, height=16386, border=2) == 0
    assert out.capacity_points == 16 * 16382 * 16382 and out.index_available == 0


def test_border_wider_than_the_frame_is_no_error():
    for border in (19, 35, 16384):
        g = d2pc.rig_geometry(d2pc.rig_config_init(n_cameras=4, width=70, height=37), border)
        assert (g.roi_points, g.capacity_points) == (0, 0) == (d2pc.roi_points(70, 37, border), 0)
        assert g.device_bytes > 0 and g.index_available == 1


def _compose_numpy(t, q):
    """The association the header states, in numpy float64 (no fused multiply-add: every product is rounded into an
    array before it is added)."""
    t, q = np.asarray(t, dtype=np.float64).reshape(4, 4), np.asarray(q, dtype=np.float64).reshape(4, 4)
    out = np.empty((4, 4))
    for r in range(4):
        for k in range(4):
            p = [np.float64(t[r, j]) * np.float64(q[j, k]) for j in range(4)]
            out[r, k] = ((p[0] + p[1]) + p[2]) + p[3]
    return out


def test_compose_q_bit_equal_to_the_stated_association():
    rng = np.random.default_rng(72)
    for trial in range(200):
        t = rng.normal(size=(4, 4)) * 10.0 ** rng.integers(-3, 4, size=(4, 4))
        q = rng.normal(size=(4, 4)) * 10.0 ** rng.integers(-3, 4, size=(4, 4))
        if trial % 3 == 0:   # a pose in front of a stereoRectify Q
            a = rng.uniform(0, 2 * np.pi)
            t = np.array([[np.cos(a), 0, np.sin(a), rng.normal()], [0, 1, 0, rng.normal()],
                          [-np.sin(a), 0, np.cos(a), rng.normal()], [0, 0, 0, 1]])
            q = d2pc.make_q(fx=rng.uniform(300, 900), cx=rng.uniform(100, 600)).reshape(4, 4)
        got = d2pc.rig_compose_q(t, q)
        want = _compose_numpy(t, q)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), trial


def test_identity_pose_keeps_the_q():
    q = d2pc.make_q()
    got = d2pc.rig_compose_q(np.eye(4), q).reshape(16)
    assert np.array_equal(got, q)   # == element-wise ...
    changed = np.flatnonzero(got.view(np.uint64) != q.view(np.uint64))
    assert list(changed) == [15] and np.signbit(q[15]) and not np.signbit(got[15])   # ... only -0.0 became +0.0
    # in place, either argument
    a, b = np.eye(4).reshape(16).copy(), q.copy()
    dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    assert d2pc.load_library().d2pc_rig_compose_q(dp(a), dp(b), dp(b)) == 0 and np.array_equal(b, got)


def test_compose_q_refuses_non_finite_and_null():
    q, t = d2pc.make_q(), np.eye(4)
    for bad in (np.nan, np.inf, -np.inf):
        for which in (0, 1):
            for at in (0, 7, 15):
                args = [t.copy().reshape(16), q.copy()]
                args[which][at] = bad
                with pytest.raises(d2pc.D2pcError) as e:
                    d2pc.rig_compose_q(*args)
                assert e.value.status == INVALID_ARG
    L = d2pc.load_library()
    dp = q.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.d2pc_rig_compose_q(None, dp, dp) == L.d2pc_rig_compose_q(dp, None, dp) == L.d2pc_rig_compose_q(dp, dp, None) == INVALID_ARG
    # a T that is not rigid is the caller's business
    assert np.array_equal(d2pc.rig_compose_q(2.0 * np.eye(4), q).reshape(16), 2.0 * q)


def test_rig_symbols_are_bound_and_exported():
    L = d2pc.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    for name in RIG_SYMBOLS:
        assert name in capi.ABI_SYMBOLS and name in exported and hasattr(L, name), name
    assert sorted(s for s in capi.ABI_SYMBOLS if s.startswith("d2pc_rig_")) == sorted(RIG_SYMBOLS)


def test_null_rig_calls_return_invalid_arg():
    L = d2pc.load_library()
    q = d2pc.make_q()
    dp = q.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    cfg = d2pc.rig_config_init(width=8, height=8)
    h = ctypes.c_void_p()
    assert L.d2pc_rig_create(None, ctypes.byref(cfg), dp, ctypes.byref(h)) == INVALID_ARG
    assert L.d2pc_rig_set_q(None, 0, dp) == L.d2pc_rig_get_q(None, 0, dp) == L.d2pc_rig_destroy(None) == INVALID_ARG
    assert L.d2pc_rig_process_device(None, None, 1.0, 0, 0, None, None, 0, None, None, None) == INVALID_ARG
