"""CPU tests of the textured-cloud surface (d2pc_texture_*, include/d2pc.h): symbols, struct layouts, the host-only
metadata, the refusals that need no device, the expected-bytes helper against a committed blob.  No compute call: the
library has no CPU path.  tests/README_textured.md lists what the GPU file covers."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import textured_expect as te
from disparity_to_point_cloud_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, BAD_DTYPE, BAD_SIZE = 1, 2, 3
NEW = ("d2pc_texture_desc_init", "d2pc_texture_device", "d2pc_textured_cloud_meta_fill")


def test_symbols_are_exported_and_bound():
    lib = d2pc.load_library()
    header = open(os.path.join(ROOT, "include", "d2pc.h")).read()
    for name in NEW:
        assert name in capi.ABI_SYMBOLS and hasattr(lib, name) and name + "(" in header
    assert lib.d2pc_abi_version() == 2          # additions only
    assert (d2pc.POINT_XYZI, d2pc.POINT_XYZRGB) == (te.POINT_XYZI, te.POINT_XYZRGB) == (1, 2)
    assert (d2pc.TEX_U8, d2pc.TEX_U16, d2pc.TEX_F32, d2pc.TEX_RGB8, d2pc.TEX_BGR8, d2pc.TEX_MONO8) == (1, 2, 3, 4, 5, 6)
    for name, value in (("D2PC_POINT_XYZI", 1), ("D2PC_POINT_XYZRGB", 2), ("D2PC_TEX_U8", 1), ("D2PC_TEX_U16", 2),
                        ("D2PC_TEX_F32", 3), ("D2PC_TEX_RGB8", 4), ("D2PC_TEX_BGR8", 5), ("D2PC_TEX_MONO8", 6)):
        assert "%s = %d" % (name, value) in header


def test_struct_sizes_and_desc_init_defaults():
    assert ctypes.sizeof(capi.TextureDesc) == 112
    assert ctypes.sizeof(capi.TexturedField) == 24 and ctypes.sizeof(capi.TexturedCloudMeta) == 120
    d = capi.TextureDesc()
    ctypes.memset(ctypes.byref(d), 0xFF, ctypes.sizeof(d))
    d2pc.load_library().d2pc_texture_desc_init(ctypes.byref(d))
    assert (d.struct_size, d.point_format, d.texture_format, d.n_frames) == (112, d2pc.POINT_XYZI, d2pc.TEX_U8, 1)
    for name, _ in capi.TextureDesc._fields_:
        if name not in ("struct_size", "point_format", "texture_format", "n_frames"):
            assert not getattr(d, name), name
    d2pc.load_library().d2pc_texture_desc_init(None)   # tolerated, like the other *_init
    with pytest.raises(TypeError):
        d2pc.texture_desc_init(no_such_field=1)


def test_the_c_compiler_agrees_on_the_layouts(tmp_path):
    """d2pc.h still compiles as strict C99 and C++11 with the new declarations in use, and sizeof / offsetof are what
    the ctypes structures assume."""
    src = tmp_path / "tex.c"
    src.write_text(
        '#include <stddef.h>\n#include "d2pc.h"\n'
        'typedef char a0[sizeof(d2pc_texture_desc) == 112 ? 1 : -1];\n'
        'typedef char a1[offsetof(d2pc_texture_desc, texture) == 32 ? 1 : -1];\n'
        'typedef char a2[offsetof(d2pc_texture_desc, cloud_points) == 80 ? 1 : -1];\n'
        'typedef char a3[offsetof(d2pc_texture_desc, out_frame_stride_points) == 104 ? 1 : -1];\n'
        'typedef char a4[sizeof(d2pc_textured_field) == 24 ? 1 : -1];\n'
        'typedef char a5[sizeof(d2pc_textured_cloud_meta) == 120 ? 1 : -1];\n'
        'typedef char a6[offsetof(d2pc_textured_cloud_meta, fields) == 24 ? 1 : -1];\n'
        'int main(void) { d2pc_texture_desc d; d2pc_textured_cloud_meta m; d2pc_texture_desc_init(&d);\n'
        '  d.point_format = D2PC_POINT_XYZRGB; d.texture_format = D2PC_TEX_BGR8;\n'
        '  return d2pc_textured_cloud_meta_fill(D2PC_POINT_XYZI, 4, 0, &m) + d2pc_texture_device(NULL, &d, NULL); }\n')
    inc = os.path.join(ROOT, "include")
    for cmd in (["gcc", "-std=c99"], ["g++", "-std=c++11", "-x", "c++"]):
        p = subprocess.run(cmd + ["-pedantic", "-Wall", "-Wextra", "-Werror", "-I", inc, "-c", str(src), "-o",
                                  str(tmp_path / "tex.o")], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
    assert capi.TextureDesc.texture.offset == 32 and capi.TextureDesc.cloud_points.offset == 80
    assert capi.TextureDesc.out_frame_stride_points.offset == 104 and capi.TexturedCloudMeta.fields.offset == 24


def meta_bytes(name4, n, dense):
    """d2pc_textured_cloud_meta as the header lays it out, built by hand (little endian, padding zero)."""
    b = np.zeros(120, dtype=np.uint8)
    b[0:16] = np.array([1, n, 32, 32 * n], dtype="<u4").view(np.uint8)
    b[16], b[17] = 0, dense
    b[20:24] = np.array([4], dtype="<u4").view(np.uint8)
    for i, (name, off) in enumerate((("x", 0), ("y", 4), ("z", 8), (name4, 16))):
        o = 24 + 24 * i
        b[o:o + len(name)] = np.frombuffer(name.encode(), dtype=np.uint8)
        b[o + 12:o + 16] = np.array([off], dtype="<u4").view(np.uint8)
        b[o + 16] = 7
        b[o + 20:o + 24] = np.array([1], dtype="<u4").view(np.uint8)
    return b.tobytes()


@pytest.mark.parametrize("fmt,name4", [(1, "intensity"), (2, "rgb")])
def test_textured_cloud_meta_fill_byte_for_byte(fmt, name4):
    lib = d2pc.load_library()
    for n, dense in ((4, 0), (0, 1), (268800, 1), ((1 << 27) - 1, 0)):
        m = capi.TexturedCloudMeta()
        ctypes.memset(ctypes.byref(m), 0xEE, ctypes.sizeof(m))
        assert lib.d2pc_textured_cloud_meta_fill(fmt, n, dense * 5, ctypes.byref(m)) == 0
        assert bytes(m) == meta_bytes(name4, n, dense), (fmt, n)
    m = d2pc.textured_cloud_meta(fmt, 7, True)
    assert (m.point_step, m.row_step, m.is_dense, m.fields[3].name.decode(), m.fields[3].offset) == (32, 224, 1, name4, 16)
    keep = bytes(m)
    assert lib.d2pc_textured_cloud_meta_fill(fmt, 1 << 27, 0, ctypes.byref(m)) == BAD_SIZE     # 32 n needs 33 bits
    assert lib.d2pc_textured_cloud_meta_fill(0, 4, 0, ctypes.byref(m)) == BAD_DTYPE
    assert lib.d2pc_textured_cloud_meta_fill(3, 4, 0, ctypes.byref(m)) == BAD_DTYPE
    assert lib.d2pc_textured_cloud_meta_fill(fmt, 4, 0, None) == INVALID_ARG
    assert bytes(m) == keep, "a refusal wrote the meta"
    with pytest.raises(d2pc.D2pcError):
        d2pc.textured_cloud_meta(9, 4, False)


def test_null_arguments_are_refused_without_a_device():
    lib = d2pc.load_library()
    d = d2pc.texture_desc_init()
    assert lib.d2pc_texture_device(None, ctypes.byref(d), None) == INVALID_ARG
    assert lib.d2pc_texture_device(None, None, None) == INVALID_ARG


def test_xyzi_blob_82x82(golden_dir):
    """The committed blob equals what the helper builds from the committed XYZ blob, and the library's meta describes
    it."""
    import sys
    sys.path.insert(0, golden_dir)
    import make_textured_golden as gen

    base = json.load(open(os.path.join(golden_dir, "pointcloud2_82x82.json")))
    gold = json.load(open(os.path.join(golden_dir, "pointcloud2_xyzi_82x82.json")))
    blob = bytes.fromhex(gold["data_hex"])
    assert len(blob) == gold["row_step"] == gold["point_step"] * gold["width"] == 128
    rec = np.frombuffer(blob, dtype=np.uint32).reshape(4, 8)
    assert rec[:, :4].tobytes() == bytes.fromhex(base["data_hex"])
    assert np.array_equal(rec[:, 4].view(np.float32), np.array(gold["roi_intensities"], dtype=np.float32))
    assert gold["roi_intensities"] == [(7 * v + 13 * u + 5) % 256 for v in (40, 41) for u in (40, 41)]
    assert not rec[:, 5:].any() and np.all(rec[:, 3] == 0x3F800000)
    tex = gen.texture_82x82()
    assert np.array_equal(te.expect_records(rec[:, :4], te.roi_pixels(82, 82, 40), tex[None], "u8", frame=0), rec)
    m = d2pc.textured_cloud_meta(d2pc.POINT_XYZI, 4, False)
    assert (m.height, m.width, m.point_step, m.row_step) == (gold["height"], gold["width"], gold["point_step"], gold["row_step"])
    assert (m.is_bigendian, m.is_dense, m.n_fields) == (0, 0, len(gold["fields"]))
    for f, ref in zip(m.fields, gold["fields"]):
        assert (f.name.decode(), f.offset, f.datatype, f.count) == (ref["name"], ref["offset"], ref["datatype"], ref["count"])


def test_expected_bytes_helper():
    """The helper itself, on values written out by hand."""
    pts = np.array([[1, 2, 3, 0x3F800000], [0x7FC00123, 0x80000000, 0xFF800000, 0x3F800000]], dtype=np.uint32)
    rgb = np.zeros((2, 2, 3, 3), dtype=np.uint8)
    rgb[1, 1, 2] = (0x11, 0x22, 0x33)
    pix = np.array([0, 1 * 6 + 1 * 3 + 2])
    assert te.expect_records(pts, pix, rgb, "rgb8")[:, 4].tolist() == [0xFF000000, 0xFF112233]
    assert te.expect_records(pts, pix, rgb, "bgr8")[:, 4].tolist() == [0xFF000000, 0xFF332211]
    assert te.expect_records(pts, pix, rgb, "rgb8", n_declared=1)[:, 4].tolist() == [0xFF000000, 0]
    assert te.expect_records(pts, [5, 6], rgb, "rgb8", frame=1)[:, 4].tolist() == [0xFF112233, 0]
    u16 = np.array([[[0, 65535], [256, 1]]], dtype=np.uint16)
    got = te.expect_records(pts, [1, 2], u16, "u16")
    assert got[:, 4].view(np.float32).tolist() == [65535.0, 256.0] and np.array_equal(got[:, :4], pts) and not got[:, 5:].any()
    f32 = np.array([[[0x7FC0BEEF, 0x80000000]]], dtype=np.uint32).view(np.float32)
    assert te.expect_records(pts, [0, 1], f32, "f32")[:, 4].tolist() == [0x7FC0BEEF, 0x80000000]
    assert te.expect_records(pts, [0, 1], np.array([[[7, 200]]], dtype=np.uint8), "mono8")[:, 4].tolist() == [0xFF070707, 0xFFC8C8C8]
    assert te.roi_pixels(4, 5, 1).tolist() == [6, 7, 8, 11, 12, 13]
