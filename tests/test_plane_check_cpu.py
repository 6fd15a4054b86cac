"""csrc/d2pc_plane.hpp -- the one plane checker in front of the image entry points of the C ABI -- without a GPU:
tests/cpp/plane_check_main.cpp enumerates every small plane (row bytes 1..4, rows 1..3, pitch 0..6, frames 1..3, frame
stride 0..20, bases 0..40 of a 256-byte arena), marks the bytes it touches and compares extent, the fit test (both
32-bit bounds, both frame-stride rules), overlaps and kernel_frame_stride with what the marks say; plus the 2^32 edges.
Built with plain g++ under ASan + UBSan: the header includes nothing of HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plane_helper_against_a_byte_by_byte_model(tmp_path):
    exe = tmp_path / "plane_check"
    src = os.path.join(ROOT, "tests", "cpp", "plane_check_main.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-o", str(exe), src], check=True, capture_output=True, timeout=180)
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0 and "plane check ok" in p.stdout, p.stdout + p.stderr
    planes, pairs = (int(p.stdout.split()[i]) for i in (3, 5))
    assert planes == 4 * 3 * 7 * 3 * 21 * 41 and 400_000 < pairs < 1_000_000, p.stdout
