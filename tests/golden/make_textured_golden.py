"""Writes pointcloud2_xyzi_82x82.json: the PointCloud2 of pointcloud2_82x82.json's four points (an 82 x 82 frame, default
Q, border 40) as pcl::PointXYZI records, the intensity taken from an 8-bit texture of the same frame.  The xyz bytes
are the committed ones of pointcloud2_82x82.json; the rest is tests/textured_expect.py.  Run from anywhere:
    python tests/golden/make_textured_golden.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import textured_expect as te  # noqa: E402


def texture_82x82():
    """8-bit texture whose four ROI pixels differ from each other and from their neighbours."""
    v, u = np.mgrid[0:82, 0:82]
    return ((7 * v + 13 * u + 5) % 256).astype(np.uint8)


def main():
    base = json.load(open(os.path.join(HERE, "pointcloud2_82x82.json")))
    pts = np.frombuffer(bytes.fromhex(base["data_hex"]), dtype=np.uint32).reshape(-1, 4)
    tex = texture_82x82()
    rec = te.expect_records(pts, te.roi_pixels(82, 82, 40), tex[None], "u8", frame=0)
    meta = {
        "comment": "pointcloud2_82x82.json's 4 points as pcl::PointXYZI, intensity = (7 v + 13 u + 5) % 256 of the pixel",
        "roi_intensities": [int(x) for x in tex[40:42, 40:42].reshape(-1)],
        "width": 4,
        "height": 1,
        "point_step": 32,
        "row_step": 128,
        "is_bigendian": False,
        "is_dense": False,
        "fields": [
            {"name": "x", "offset": 0, "datatype": 7, "count": 1},
            {"name": "y", "offset": 4, "datatype": 7, "count": 1},
            {"name": "z", "offset": 8, "datatype": 7, "count": 1},
            {"name": "intensity", "offset": 16, "datatype": 7, "count": 1},
        ],
        "frame_id": base["frame_id"],
        "data_hex": rec.tobytes().hex(),
    }
    with open(os.path.join(HERE, "pointcloud2_xyzi_82x82.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("pointcloud2_xyzi_82x82.json", rec.nbytes, "bytes")


if __name__ == "__main__":
    main()
