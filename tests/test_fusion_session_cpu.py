"""The C-ABI session of the depth_map_fusion node (d2pc_fusion_node_*) without a GPU: struct layouts against the
header, the defaults, the host arithmetic of d2pc_fusion_node_geometry, the refusals that need no device, the header
as strict C99 / C++11, the ROS adaptor's syntax check and the replay harness's refusals."""
import ctypes
import os
import subprocess

import pytest

import disparity_to_point_cloud_amd as d2pc
from disparity_to_point_cloud_amd import capi
import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
REPLAY = os.path.join(ROOT, "host", "d2pc_replay")

STRUCTS = {"d2pc_fusion_node_config": capi.FusionNodeConfig, "d2pc_fusion_node_geometry_t": capi.FusionNodeGeometry,
           "d2pc_fusion_node_topic": capi.FusionNodeTopic, "d2pc_fusion_node_topics": capi.FusionNodeTopics,
           "d2pc_fusion_node_host_topics": capi.FusionNodeHostTopics}


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof and every offsetof, printed by a C program compiled against include/d2pc.h."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "d2pc.h"', 'int main(void) {']
    for cname, cls in STRUCTS.items():
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{field} %zu\\n", offsetof({cname}, {field}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    p = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", INC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    n = 0
    for cname, cls in STRUCTS.items():
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for field, _ in cls._fields_:
            assert int(got[f"{cname}.{field}"]) == getattr(cls, field).offset, (cname, field)
            n += 1
    assert n == sum(len(c._fields_) for c in STRUCTS.values()) >= 40


def test_config_init_gives_the_reference_values():
    c = d2pc.fusion_node_config_init()
    assert c.struct_size == ctypes.sizeof(capi.FusionNodeConfig)
    assert (c.offset_x, c.offset_y) == (0, 0)                      # the class defaults (hpp:92-93), not the launch file's
    assert c.rule == d2pc.FUSE_GRAD_FILTER and c.score_form == d2pc.SCORE_FORM_CV4 and c.batch == 1
    assert (c.crop_left, c.crop_right, c.crop_top, c.crop_bottom) == (0, 40, 30, 10)   # cpp:130
    assert c.single_launch == 1
    assert (c.cols, c.rows) == (0, 0) and list(c.reserved) == [0, 0, 0]
    d2pc.load_library().d2pc_fusion_node_config_init(None)         # a null pointer is ignored
    assert [capi.NODE_DISPARITY_1, capi.NODE_DISPARITY_2, capi.NODE_MATCHING_SCORE_1, capi.NODE_MATCHING_SCORE_2] == [0, 1, 2, 3]
    assert capi.NODE_TOPICS == ("cropped_depth_1", "cropped_depth_2", "cropped_score_1", "cropped_score_2",
                                "fused_depth_map", "combined_score", "gradient")


@pytest.mark.parametrize("cols,rows,ox,oy", [(752, 480, -7, 15), (480, 752, 7, -15), (640, 480, 0, 0), (480, 640, 0, 0),
                                             (100, 100, 3, -4), (100, 100, 0, 0), (188, 120, -2, 4), (65, 57, 1, 1)])
def test_geometry_equals_the_oracle(cols, rows, ox, oy):
    """The arithmetic of FusionNode.__init__: camera 1's square, camera 2's of the rotated frame with the negated
    offsets and the member offset_y's side length, the crop of :130."""
    for batch in (1, 5):
        g = d2pc.fusion_node_geometry(d2pc.fusion_node_config_init(cols=cols, rows=rows, offset_x=ox, offset_y=oy, batch=batch))
        assert (g.x1, g.y1, g.n) == oracle.crop_to_square(cols, rows, ox, oy)
        assert (g.x2, g.y2, g.n) == oracle.crop_to_square(rows, cols, -ox, -oy, oy)
        n = g.n
        assert (g.fused_width, g.fused_height) == (n - 40, n - 40)
        sq, fu = n * n * batch, (n - 40) * (n - 40) * batch
        assert list(g.topic_bytes) == [3 * sq, 3 * sq, sq, sq, fu, sq, 3 * fu]
    if (cols, rows, ox, oy) == (752, 480, -7, 15):
        assert (g.n, g.fused_width, g.fused_height) == (465, 425, 425)


def test_geometry_refusals():
    lib = d2pc.load_library()
    g = capi.FusionNodeGeometry()

    def status(**kw):
        c = d2pc.fusion_node_config_init(**{"cols": 188, "rows": 120, **kw})
        return lib.d2pc_fusion_node_geometry(ctypes.byref(c), ctypes.byref(g))

    assert status() == 0
    assert status(cols=10, rows=10) == 3                     # n < 11: the score filter's halo
    assert status(cols=50, rows=50) == 0 and status(cols=50, rows=50, crop_left=10) == 3    # 50 - 10 - 40: nothing left
    assert status(cols=40, rows=40) == 3                     # the default crop leaves nothing of 40 x 40
    assert status(cols=60, rows=60, crop_top=25, crop_bottom=35) == 3
    assert status(cols=100, rows=100, offset_x=0, offset_y=20) == 0   # (the member offset_y is the argument here: the square fits)
    # |offset_x| > |offset_y|: the reference fuses a smaller square than it publishes; refused
    assert status(offset_x=5, offset_y=-4) == 3 and status(offset_x=-1, offset_y=0) == 3
    assert status(offset_x=4, offset_y=-5) == 0 and status(offset_x=-5, offset_y=5) == 0 and status(offset_x=0, offset_y=-9) == 0
    assert status(cols=0) == 3 and status(rows=-1) == 3 and status(batch=0) == 3 and status(batch=70000) == 3
    assert status(crop_right=-1) == 3
    assert status(rule=9) == 1 and status(rule=-1) == 1 and status(score_form=5) == 1        # bad enums
    with pytest.raises(d2pc.D2pcError) as e:
        d2pc.fusion_node_geometry(d2pc.fusion_node_config_init(cols=10, rows=10))
    assert e.value.status == 3
    # the two squares differ in size: impossible by the arithmetic (both sides are min(cols, rows) - max(|ox|, |oy|)),
    # checked over a grid so that the refusal in the library stays dead code
    for cols in (30, 47, 64):
        for rows in (30, 51):
            for ox in (-5, 0, 4):
                for oy in (-6, 0, 3):
                    try:
                        a = oracle.crop_to_square(cols, rows, ox, oy)
                        b = oracle.crop_to_square(rows, cols, -ox, -oy, oy)
                    except Exception:
                        continue
                    assert a[2] == b[2]


def test_invalid_arguments_without_a_gpu():
    lib = d2pc.load_library()
    g, c = capi.FusionNodeGeometry(), d2pc.fusion_node_config_init(cols=188, rows=120)
    assert lib.d2pc_fusion_node_geometry(None, ctypes.byref(g)) == 1
    assert lib.d2pc_fusion_node_geometry(ctypes.byref(c), None) == 1
    bad = capi.FusionNodeConfig.from_buffer_copy(c)
    bad.struct_size = 12
    assert lib.d2pc_fusion_node_geometry(ctypes.byref(bad), ctypes.byref(g)) == 1
    h = ctypes.c_void_p()
    assert lib.d2pc_fusion_node_create(None, ctypes.byref(c), ctypes.byref(h)) == 1      # null context
    assert lib.d2pc_fusion_node_destroy(None) == 1
    out = capi.FusionNodeTopics()
    out.struct_size = ctypes.sizeof(out)
    io = capi.FusionNodeHostTopics()
    io.struct_size = ctypes.sizeof(io)
    frame = (ctypes.c_uint8 * 64)()
    for which in (0, 3, 4, -1):   # a null node, with good and bad `which`
        assert lib.d2pc_fusion_node_callback_device(None, which, frame, 8, 0, ctypes.byref(out), None) == 1
        assert lib.d2pc_fusion_node_callback(None, which, frame, 8, ctypes.byref(io)) == 1
    junk = (ctypes.c_uint8 * 1024)()                                                     # garbage in place of a node
    assert lib.d2pc_fusion_node_callback_device(ctypes.addressof(junk), 0, frame, 8, 0, ctypes.byref(out), None) == 1
    assert lib.d2pc_fusion_node_callback(ctypes.addressof(junk), 0, frame, 8, ctypes.byref(io)) == 1
    assert lib.d2pc_fusion_node_destroy(ctypes.addressof(junk)) == 1
    if d2pc.device_count() == 0:
        with pytest.raises(d2pc.D2pcError):   # no CPU path: without a device there is no context to make a node on
            d2pc.Context()


def test_header_with_the_session_is_plain_c99_and_cxx11(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "d2pc.h"\nint main(void) { d2pc_fusion_node_config c; d2pc_fusion_node_geometry_t g; '
                   'd2pc_fusion_node_topic t; d2pc_fusion_node_topics ts; d2pc_fusion_node_host_topics hs; d2pc_fusion_node *n = 0; '
                   '(void)c; (void)g; (void)t; (void)ts; (void)hs; (void)n; '
                   'return D2PC_ABI_VERSION == 2 && D2PC_NODE_TOPICS == 7 && D2PC_TOPIC_GRADIENT == 6 && '
                   'D2PC_NODE_MATCHING_SCORE_2 == 3 ? 0 : 1; }\n')
    for cmd in (["gcc", "-std=c99"], ["g++", "-std=c++11", "-x", "c++"]):
        p = subprocess.run(cmd + ["-pedantic", "-Wall", "-Wextra", "-Werror", "-I", INC, "-c", str(src), "-o",
                                  str(tmp_path / "hdr.o")], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr


def test_abi_version_stays_2_and_the_binding_lists_the_session():
    assert d2pc.abi_version() == 2
    for name in ("d2pc_fusion_node_config_init", "d2pc_fusion_node_geometry", "d2pc_fusion_node_create",
                 "d2pc_fusion_node_destroy", "d2pc_fusion_node_callback_device", "d2pc_fusion_node_callback"):
        assert name in capi.ABI_SYMBOLS and hasattr(d2pc.load_library(), name)


def test_ros_fusion_adaptor_parses():
    """SYNTAX CHECK ONLY, as tests/test_abi_cpu.py::test_ros_adaptor_parses: ros/depth_map_fusion_node.cpp against the
    declaration-only stubs under tests/stubs/."""
    src = os.path.join(ROOT, "ros", "depth_map_fusion_node.cpp")
    p = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I",
                        os.path.join(ROOT, "tests", "stubs"), src], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    text = open(src).read()
    for topic in ("/disparity_1", "/disparity_2", "/matching_score_1", "/matching_score_2", "/cropped_depth_1",
                  "/cropped_depth_2", "/cropped_score_1", "/cropped_score_2", "/fused_depth_map", "/combined_score",
                  "/gradient", "offset_x", "offset_y", '"depth_map_fusion"'):
        assert topic in text, topic
    # the mirror binds the stable header only
    assert "d2pc_ext.h" not in open(os.path.join(ROOT, "host", "depth_map_fusion_amd.hpp")).read()
    assert "d2pc_ext.h" not in text


def test_replay_fusion_refuses_malformed_scripts(tmp_path):
    """Exit 2 before any device is touched (this runs without a GPU)."""
    assert os.path.exists(REPLAY), "host/d2pc_replay is not built"
    frame = tmp_path / "f.raw"
    frame.write_bytes(bytes(20 * 12))

    def run(script_text, *extra, size=("20", "12"), enc="mono8"):
        script = tmp_path / "script.txt"
        script.write_text(script_text)
        return subprocess.run([REPLAY, "fusion", str(script), size[0], size[1], enc, str(tmp_path / "out")] + list(extra),
                              capture_output=True, text=True, timeout=60)

    for bad in ("XX f.raw\n", "D1\n", "D1 missing.raw\n", "D1 f.raw 20\n", "D1 f.raw 20 x\n", "D1 f.raw 20 12 9\n",
                "D1 f.raw 21 12\n",     # the file is too short for that size
                "# only a comment\n\n", "D1 f.raw\nS3 f.raw\n"):
        p = run(bad)
        assert p.returncode == 2, (bad, p.returncode, p.stderr)
        assert "fusion:" in p.stderr
    assert run("D1 f.raw\n", size=("0", "12")).returncode == 2
    assert run("D1 f.raw\n", enc="rgb8").returncode == 2
    p = subprocess.run([REPLAY, "fusion", str(tmp_path / "nowhere.txt"), "20", "12", "mono8", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 2
    assert not list(tmp_path.glob("out*")), "a refused script wrote output"
