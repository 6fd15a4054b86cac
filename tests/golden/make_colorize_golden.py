#!/usr/bin/env python3
"""Known answers for colorizeDepth (src/depth_map_fusion.cpp:306-360).

NOT outputs of the reference (it cannot be built here): the 256 x 3 table derived entry by entry with scalar
np.float32 operations (one rounding per operation, as IEEE float32 code with FLT_EVAL_METHOD 0 evaluates the
chain), independent of the vectorised derivation in tests/colorize_ref.py, plus the same chain in exact rational
arithmetic so that the entries where float32 rounding shows are on record.

Stored: table (256,3) u8; d, H, hi (256,) per entry; exact (256,3) u8; differs (k,) the g whose rows differ.
Run:  python tests/golden/make_colorize_golden.py   (pure python + numpy) -> colorize_table.npz
"""
import os
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
f32 = np.float32


def entry(g, exact):
    d = int(40 + 0.8 * g)  # double, truncated to unsigned char (40 .. 244)
    H = 255 - (255 - d) * 280 // 255
    hi = (H // 60) % 6
    if exact:
        f = Fraction(H, 60) - H // 60
        one, zero, c255 = Fraction(1), Fraction(0), Fraction(255)
    else:
        f = f32(f32(H) / f32(60.0)) - f32(H // 60)
        assert type(f) is np.float32
        one, zero, c255 = f32(1.0), f32(0.0), f32(255.0)
    p, V = zero, one
    q = one - f
    t = one - (one - f)
    x, y, z = {0: (p, t, V), 1: (p, V, q), 2: (t, V, p), 3: (V, q, p), 4: (V, p, t), 5: (q, p, V)}[hi]
    row = []
    for v in (x, y, z):
        v = max(zero, min(v, one)) * c255
        assert exact or type(v) is np.float32
        row.append(int(v))  # truncation (the value is >= 0)
    if d == 40:
        row = [0, 0, 0]
    return d, H, hi, row


def main():
    cols = {k: [] for k in ("d", "H", "hi", "table", "exact")}
    for g in range(256):
        d, H, hi, row = entry(g, exact=False)
        cols["d"].append(d), cols["H"].append(H), cols["hi"].append(hi), cols["table"].append(row)
        cols["exact"].append(entry(g, exact=True)[3])
    table, exact = np.array(cols["table"], np.uint8), np.array(cols["exact"], np.uint8)
    differs = np.flatnonzero((table != exact).any(axis=1)).astype(np.int32)
    np.savez_compressed(os.path.join(HERE, "colorize_table.npz"), table=table, exact=exact, differs=differs,
                        d=np.array(cols["d"], np.int32), H=np.array(cols["H"], np.int32), hi=np.array(cols["hi"], np.int32))
    print("colorize_table.npz: %d entries differ from exact arithmetic: %s" % (len(differs), differs.tolist()))


if __name__ == "__main__":
    main()
