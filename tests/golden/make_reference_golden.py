#!/usr/bin/env python3
"""Recorded runs of the COMPILED reference node (oracle/ref.py: the reference's unmodified depth_map_fusion.cpp against
the stand-ins of oracle/ref_shim/, its three OpenCV filters supplied by tests/ref_filters.py) -> reference_fusion.npz.

For every script of tests/ref_frames.py SCRIPTS, callback by callback, what the reference published, in its order:
  index                       JSON: per script its geometry, score form, callbacks and, per callback, the list of
                              [topic, encoding, width, height, step, sha256 of the bytes]
  <script>/in/<i>             the input frame of callback i            } the small scripts only; the larger ones
  <script>/out/<i>/<topic>    the published bytes as an array          } regenerate their frames (ref_frames.frame)
                                                                         and keep the digests alone
Needs oracle/_ref/libref_fusion.so, that is, a machine with the reference's sources (oracle.build()).
Run:  python tests/golden/make_reference_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if p not in sys.path:
        sys.path.insert(0, p)

import ref_filters  # noqa: E402
import ref_frames  # noqa: E402
from oracle import ref  # noqa: E402


def record(name):
    """-> (index entry, {key: array}) of one script."""
    cols, rows, ox, oy, form, _, calls, stored = ref_frames.SCRIPTS[name]
    ref_filters.install(form)
    node = ref.Node(ox, oy)
    arrays, published = {}, []
    for i, (call, f) in enumerate(zip(calls, ref_frames.script_frames(name))):
        topics = node.callback(call, f)
        published.append([[t.lstrip("/"), enc, w, h, step, ref_frames.digest(data)] for t, enc, w, h, step, data in topics])
        if stored:
            arrays["%s/in/%d" % (name, i)] = f
            for t, enc, w, h, step, data in topics:
                arrays["%s/out/%d/%s" % (name, i, t.lstrip("/"))] = ref_frames.topic_array(enc, w, h, data).copy()
    node.close()
    entry = {"cols": cols, "rows": rows, "offset_x": ox, "offset_y": oy, "form": form, "calls": list(calls),
             "stored": bool(stored), "published": published}
    return entry, arrays


def generate():
    index, arrays = {}, {}
    for name in ref_frames.SCRIPTS:
        index[name], a = record(name)
        arrays.update(a)
    arrays["index"] = np.frombuffer(json.dumps(index, sort_keys=True).encode(), dtype=np.uint8).copy()
    return arrays


def main():
    arrays = generate()
    path = os.path.join(HERE, "reference_fusion.npz")
    np.savez_compressed(path, **arrays)
    print("reference_fusion.npz: %d arrays, %d bytes" % (len(arrays), os.path.getsize(path)))


if __name__ == "__main__":
    main()
