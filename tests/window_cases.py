"""Built inputs for the two window sessions, the relief (d2pc_sectors_relief_*) and the terrain (d2pc_sectors_terrain_*) of
include/d2pc_sectors.h.  No GPU, no test functions: tests/test_window_cases.py asserts on the CPU that every input reaches
the edge it names, tests/test_sectors_relief_values_gpu.py and tests/test_sectors_terrain_values_gpu.py run them on the device.

(a) FIT CELLS SPREAD OVER A WINDOW.  Every cell of tests/slope_fit_cases.py (CASES and LOST) becomes a WindowCase: the points of
one WORLD cell dealt over frames that each sit at a corner of their own, so that the window of depth 4 holds exactly the
case's points at the stated update and every stored table is read at a shifted index.  Cases of one (sub, configuration) key
share a SESSION; a session runs one or more SEQUENCES of frames (a reset between them), each carrying up to six TRACKS, one
world cell each, side by side in one world row.  A track is one of
    plain   the case's points in three frames (by cluster of position); the window is the case at update 2
    evict   two cases that differ by a few points, the larger first: the difference, then the smaller case in three frames,
            then an empty frame: the window is the larger case at update 3 and the smaller at update 4 (the middle one of
            three neighbouring counts lies in two tracks, as the smaller of one and the larger of the other)
    cycle   variants of one cell that share most points: X0, A, B, empty, X1, A, B, empty, X2 -- the window always holds A, B,
            an empty frame and ONE X: variant 0 at update 3, variant 1 at updates 4 and 7, variant 2 at update 8.  A frame that
            carries the moved height enters and leaves.
The corners walk with a period of four, so the four frames of a window lie at four corners; the walk is found by a small search (corner_pattern) under the rules the CPU test asserts again.

(b) RING STATES.  A RingState describes the 16 headers, which slots hold what, one frame, and -- stated as literals, by hand
-- the replaced slot v, the new seq q and the slots that take part.  render() makes it a relief or a terrain state block.
The tables are SIGNATURES: stored slot s is entry s, the frame is entry 16; an entry's table holds bit `entry` in every
cell's count and `source cell + 1` in a field of its own: 12 bits wide, five fields to a 64-bit plane (relief: planes 0 .. 3
hold the 17 entries, planes 4 .. 7 repeat them, plane 8 holds (source cell + 1) * (entry + 1)), or 7 bits wide, nine fields
to a plane (terrain: sum and sum2 hold 17 of the 18 fields; its grids have at most 126 cells).  Every field of a window's cell
is added to at most once, so nothing carries: decode() reads from a window cell's sums alone which (entry, source cell)
pairs were added, and names the slot and the cell when they are not the expected ones.

(c) ring_copy: the anchor gate, the slot choice and the participant test in plain Python integers, every decision point a
parameter; RING_MUTATIONS lists the mutations, tests/test_window_cases.py names the state that kills each.

(d) TERRAIN EDGES: integer heights over three or more frames at shifted corners, whose window reaches an edge of the GROUND
block's cell formula (TERRAIN_EDGES), each expectation stated in exact integers."""
import itertools
import operator
from collections import Counter

import numpy as np

import sectors_ground_ref as gref
import sectors_relief_cases as rcases
import sectors_relief_ref as rref
import sectors_terrain_ref as tref
import slope_fit_cases as sfc

F32 = np.float32
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
OFF = 0xFFFFFFFF
DEPTH = 4                                        # of every session of (a)
WORLD = (100, -50)                               # the world cell of track 0 of a sequence
JUDGE = dict(max_step_q=50, window=0, w_dist=1, w_rough=1, rough_cap=65535)      # a window of 0: a flat cell is a site
TWELVE = ("count", "sum", "sum2", "slope_a", "slope_b", "level_q", "resid_q2", "flat")       # and the seven moments


# ------------------------------------------------------------------------------------------------ (a) tracks
def clusters_split(points, parts):
    """The points dealt into `parts` lists: by cluster of position (u, w) where there are enough clusters, else one by one."""
    points = sorted(points)
    where = sorted({(u, w) for u, w, _ in points})
    out = [[] for _ in range(parts)]
    for n, p in enumerate(points):
        out[(where.index((p[0], p[1])) if len(where) >= parts else n) % parts].append(p)
    return out


def minus(a, b):
    """The multiset a - b of points; b must lie in a."""
    left = Counter(a)
    left.subtract(Counter(b))
    assert min(left.values(), default=0) >= 0, "not a sub-multiset"
    return sorted(left.elements())


class Track:
    """One world cell of a sequence: its frames' points and the updates at which the window is a named case."""

    def __init__(self, kind, parts, at, unnamed=None):
        self.kind, self.parts, self.at, self.unnamed = kind, parts, at, unnamed or {}      # at: {case name: [updates]}

    def part(self, f):
        return self.parts[f] if f < len(self.parts) else []


def plain(case):
    return Track("plain", clusters_split(case.points, 3), {case.name: [2]})


def evict(cases):
    """cases[0] holds cases[1] holds ...: the differences first, then the smallest case over the frames left of DEPTH."""
    diffs = [minus(a.points, b.points) for a, b in zip(cases, cases[1:])]
    assert all(diffs) and len(cases) == 2
    parts = diffs + clusters_split(cases[-1].points, DEPTH - len(diffs)) + [[] for _ in diffs]
    return Track("evict", parts, {c.name: [DEPTH - 1 + n] for n, c in enumerate(cases)})


def cycle(variants):
    """variants: [(case or None, points)] of one cell, two or three: what they share is A and B, the rest X0, X1, X2."""
    shared = Counter(variants[0][1])
    for _, pts in variants[1:]:
        shared &= Counter(pts)
    shared = sorted(shared.elements())
    a, b = clusters_split(shared, 2)
    xs = [minus(pts, shared) for _, pts in variants]
    assert all(xs) and a and b
    parts = [xs[0], a, b, [], xs[1]] + ([a, b, [], xs[2]] if len(variants) == 3 else [])
    at, unnamed = {}, {}
    for (case, pts), updates in zip(variants, ([3], [4, 7] if len(variants) == 3 else [4], [8])):
        if case is None:
            unnamed.update({t: pts for t in updates})
        else:
            at[case.name] = updates
    return Track("cycle", parts, at, unnamed)


def spoiled(case):
    """The case's points with the first height moved up by the fewest quanta that take resid_q2 (exact least squares') above
    max_spread_q2: the neighbour a flat cell is reached from by eviction."""
    u, w, k = case.points[0]
    for dk in range(1, 400):
        pts = [(u, w, k + dk)] + case.points[1:]
        e = sfc.exact_fit(pts, sub=case.sub, **case.cfg)
        if e["fitted"] and e["resid_q2"] > case.cfg["max_spread_q2"]:
            return pts
    raise AssertionError("no such height")


def tracks_of(fam, cases):
    """The tracks of one session's cases."""
    by = {c.name: c for c in cases}
    used, out = set(), []

    def take(*names):
        used.update(names)
        return [by[n] for n in names]

    if fam == "gate":
        for chain in (("gate_one_off_fails", "gate_one_off_holds"), ("gate_two_off_fails", "gate_two_off_holds"),
                      ("gate_count_4_of_3", "gate_count_3_of_3"), ("gate_count_3_of_3", "gate_count_2_of_3"),
                      ("gate_count_8_of_7", "gate_count_7_of_7"), ("gate_count_7_of_7", "gate_count_6_of_7")):
            if chain[0] in by:
                out.append(evict(take(*chain)))
    if fam == "level":
        for tag in sfc.LEVEL_TIES:
            down, tie, up = take(*("level_%s_%s" % (tag, x) for x in ("down", "tie", "up")))
            out.append(cycle([(down, down.points), (tie, tie.points), (up, up.points)]))
    if fam == "resid":
        for c in cases:
            if c.exact()["flat"]:                                      # *_at and resid_just_below: reached from a rough neighbour
                out.append(cycle([(None, spoiled(c)), (c, c.points)]))
                used.add(c.name)
    return out + [plain(c) for c in cases if c.name not in used]


# ------------------------------------------------------------------------------------------------ (a) corners
_patterns = {}


def corner_pattern(n_a, n_b, m):
    """DEPTH different (o, j): in frame f track b lies at grid cell (b + o, j) of phase f % DEPTH, so the frames of one window
    lie at DEPTH different corners and every stored table is read at a shifted index.  The first such tuple, in a fixed order,
    under which, over updates 1 and 2, the shifts take both signs on both axes and one of them is n_a - 1 or n_b - 1 in size,
    and (on a grid of more than 16 cells) some track lies on index 15 in one frame and some track on index 16 in another: the
    seam of two blocks of k_relief_window, the second of which is the last, partly filled one."""
    if (n_a, n_b, m) in _patterns:
        return _patterns[n_a, n_b, m]
    spots = [(o, j) for j in range(n_b) for o in range(n_a - m + 1)]
    for first in itertools.permutations(spots, 3):
        shifts = [(first[f][0] - first[t][0], first[f][1] - first[t][1]) for t in (1, 2) for f in range(t)]       # stored minus current
        if not (min(d for d, _ in shifts) < 0 < max(d for d, _ in shifts) and min(d for _, d in shifts) < 0 < max(d for _, d in shifts)):
            continue
        if not any(abs(d) == n_a - 1 for d, _ in shifts) and not any(abs(d) == n_b - 1 for _, d in shifts):
            continue
        index = {j * n_a + b + o for o, j in first for b in range(m)}        # (within the first three frames: every sequence has them)
        if n_a * n_b > 16 and not {15, 16} <= index:
            continue
        for last in spots:
            if last not in first:
                _patterns[n_a, n_b, m] = first + (last,)
                return first + (last,)
    raise AssertionError("no pattern for %d x %d, %d tracks" % (n_a, n_b, m))


class Sequence:
    """Frames of one session between two resets: every track's part f lies in frame f, whose corner is corners[f]."""

    def __init__(self, fam, sub, cfg, n_a, n_b, tracks, order=None):
        self.fam, self.sub, self.cfg, self.n_a, self.n_b, self.tracks, self.depth = fam, sub, cfg, n_a, n_b, tracks, DEPTH
        self.n_frames = max(len(t.parts) for t in tracks)
        self.pattern = corner_pattern(n_a, n_b, len(tracks))
        self.cells = [(WORLD[0] + b, WORLD[1]) for b in range(len(tracks))]
        self.corners = [(WORLD[0] - self.pattern[f % DEPTH][0], WORLD[1] - self.pattern[f % DEPTH][1]) for f in range(self.n_frames)]
        self.order = list(order) if order is not None else list(range(self.n_frames))     # the frames in their order of arrival

    def index(self, f, b):
        """The grid index of track b in frame f; asserts that the frame sees it."""
        i, j = self.cells[b][0] - self.corners[f][0], self.cells[b][1] - self.corners[f][1]
        assert 0 <= i < self.n_a and 0 <= j < self.n_b
        return j * self.n_a + i

    def frame(self, f):
        """-> (the step's 20 words, (count, sum, sum2, moments)) of frame f, from sectors_relief_cases.sums_of."""
        cell, pts = [], []
        for b, t in enumerate(self.tracks):
            cell += [self.index(f, b)] * len(t.part(f))
            pts += t.part(f)
        p = np.asarray(pts, dtype=np.int64).reshape(-1, 3)
        return rcases.corner_step(*self.corners[f]), rcases.sums_of(self.n_a * self.n_b, cell, p[:, 2], p[:, 0], p[:, 1])

    def window_points(self, b, t):
        """From the frames alone: the multiset of points that the window of update t holds for track b's world cell, and the
        shifts (stored index minus current index, per axis) at which the stored frames are read."""
        pts, shifts = [], []
        for f in range(max(0, t - self.depth + 1), t + 1):
            self.index(f, b)                                          # (in sight of the frame that stored it ...)
            pts += self.tracks[b].part(f)
            if f != t:
                shifts.append((self.corners[t][0] - self.corners[f][0], self.corners[t][1] - self.corners[f][1]))
        return sorted(pts), shifts

    def reversed_window(self, t):
        """The frames of the window of update t in the reverse order of arrival, as a sequence of their own."""
        seq = Sequence(self.fam, self.sub, self.cfg, self.n_a, self.n_b, self.tracks)
        seq.order = list(range(t, t - self.depth, -1))
        return seq


class WindowCase:
    """One built cell in a window: its frames (corner, points of its world cell), the depth, and the updates at which the
    window is the case."""

    def __init__(self, case, session, seq, b):
        self.case, self.name, self.session, self.seq, self.b = case, case.name, session, seq, b
        self.track, self.depth, self.cell = seq.tracks[b], seq.depth, seq.cells[b]
        self.updates = self.track.at[case.name]
        self.frames = [(seq.corners[f], self.track.part(f)) for f in range(seq.n_frames)]
        for t in self.updates:                                        # rule 3, from the frames alone
            assert seq.window_points(b, t)[0] == sorted(case.points), "%s: the window of update %d is not the case" % (case.name, t)


class Session:
    """The sequences of one (sub, configuration) key: one relief session on the device."""

    def __init__(self, fam, sub, cfg, cases):
        self.fam, self.sub, self.cfg, self.cases = fam, sub, dict(cfg), cases
        tracks = tracks_of(fam, cases)
        self.n_a, self.n_b = (5, 3) if fam == "gate" and self.cfg["min_count"] == 7 else (8, 3)      # the one 5 x 3: gate_count_*_of_7
        most = self.n_a - 2
        self.sequences = [Sequence(fam, sub, self.cfg, self.n_a, self.n_b, tracks[i:i + most]) for i in range(0, len(tracks), most)]
        found = {}                                                    # (a case that lies in two tracks is the first one's)
        for seq in self.sequences:
            for b, t in enumerate(seq.tracks):
                for c in cases:
                    if c.name in t.at and c.name not in found:
                        found[c.name] = WindowCase(c, self, seq, b)
        self.window_cases = [found[c.name] for c in cases]

    def config(self):
        """The keywords of the ground configuration, and of the slope's, as the device's harness and relief_ref_of take them."""
        return dict(JUDGE, n_a=self.n_a, n_b=self.n_b, cell_size=sfc.CELL_SIZE, quantum=sfc.QUANTUM, min_count=self.cfg["min_count"],
                    max_spread_q2=self.cfg["max_spread_q2"]), dict(sub=self.sub, max_slope=self.cfg["max_slope"])


def sessions(fam):
    """The family's sessions by the (sub, configuration) key of slope_fit_cases.groups; lost_level_tie rides with the level ties."""
    out = []
    for (sub, items), cases in sfc.groups(fam):
        cfg = dict(items)
        extra = [sfc.LOST] if fam == "level" and (sfc.LOST.sub, sfc.LOST.cfg) == (sub, cfg) else []
        out.append(Session(fam, sub, cfg, cases + extra))
    return out


_sessions = {}


def all_sessions():
    if not _sessions:
        for fam in sfc.FAMILIES:
            _sessions[fam] = sessions(fam)
    return _sessions


def window_cases():
    return [wc for ss in all_sessions().values() for s in ss for wc in s.window_cases]


# the pairs that eviction reaches in one sequence: (the case before, the case after, the decision that flips, before, after);
# the second is read one update after the first.  A `None` before is the unnamed rough neighbour of `spoiled`.
def eviction_pairs():
    pairs = [("gate_one_off_fails", "gate_one_off_holds", "fitted"), ("gate_two_off_fails", "gate_two_off_holds", "fitted"),
             ("gate_count_3_of_3", "gate_count_2_of_3", "fitted"), ("gate_count_7_of_7", "gate_count_6_of_7", "fitted")]
    pairs += [(None, c.name, "flat") for c in sfc.family("resid") if c.exact()["flat"]]
    for tag, (c0, _, m, rc) in sfc.LEVEL_TIES.items():
        lo, mid, hi = [sfc.by_name("level_%s_%s" % (tag, x)).exact()["level_q"] for x in ("down", "tie", "up")]
        pairs.append(("level_%s_down" % tag, "level_%s_tie" % tag, "level_q") if lo != mid else ("level_%s_tie" % tag, "level_%s_up" % tag, "level_q"))
    return pairs


class Cfg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def relief_ref_of(ground, slope, depth, inv_c=None):
    """tests/sectors_relief_ref.py for the given configurations; needs no library (inv_c and inv_q are exact: powers of two)."""
    geo = Cfg(inv_c=F32(1.0 / ground["cell_size"]) if inv_c is None else F32(inv_c), inv_q=F32(1.0 / ground["quantum"]))
    return rref.SectorsReliefRef(Cfg(axes=(1, 2, 3), **ground), Cfg(**slope), geo, depth)


def terrain_ref_of(ground, depth):
    geo = Cfg(inv_c=F32(1.0 / ground["cell_size"]), inv_q=F32(1.0 / ground["quantum"]))
    return tref.SectorsTerrainRef(Cfg(axes=(1, 2, 3), **ground), geo, depth)


def words_of(out, n, cell):
    """The twelve per-cell words the fit and the window give for one cell -> a tuple of integers."""
    mom = np.asarray(out["moments"]).reshape(7, n)[:, cell]
    return tuple(int(np.asarray(out[o])[cell]) for o in TWELVE) + tuple(int(x) for x in mom)


# ------------------------------------------------------------------------------------------------ (b) signatures
FRAME_ENTRY = 16
H_ONE, H_TWO, H_PZERO, H_MZERO, H_NAN = 0x3F800000, 0x40000000, 0x00000000, 0x80000000, 0x7FC00001
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def layout(kind):
    """-> (field bits, fields per plane, planes of the table)."""
    return (12, 5, rref.WORDS) if kind == "relief" else (7, 9, 2)


def signature(kind, n, entry):
    """The table of entry `entry` (a stored slot 0 .. 15, or FRAME_ENTRY) -> (count uint32 (n), planes uint64 (planes, n))."""
    bits, per, n_planes = layout(kind)
    assert n + 1 < 1 << bits
    cell = np.arange(1, n + 1, dtype=np.uint64)
    planes = np.zeros((n_planes, n), dtype=np.uint64)
    planes[entry // per] = cell << np.uint64(bits * (entry % per))
    if kind == "relief":
        planes[4:8] = planes[0:4]
        planes[8] = cell * np.uint64(entry + 1)
    return np.full(n, 1 << entry, dtype=np.uint32), planes


def decode(kind, count, planes, cell, what=""):
    """One window cell's count and sums -> {(entry, source cell)}: what was added there, read from the sums alone."""
    bits, per, _ = layout(kind)
    got = set()
    for entry in range(FRAME_ENTRY + 1):
        field = (int(planes[entry // per][cell]) >> (bits * (entry % per))) & ((1 << bits) - 1)
        bit = (int(count[cell]) >> entry) & 1
        assert bit == (field != 0), "%s: cell %d, entry %d: the count says %d and its field holds %d" % (what, cell, entry, bit, field)
        if bit:
            got.add((entry, field - 1))
    assert int(count[cell]) >> (FRAME_ENTRY + 1) == 0, "%s: cell %d: an entry was added twice" % (what, cell)
    return got


def hand_window(n_a, n_b, parts, anchored=True):
    """{cell: {(entry, source cell)}} for the frame and the listed (slot, di, dj), in plain loops."""
    want = {}
    for j in range(n_b):
        for i in range(n_a):
            got = {(FRAME_ENTRY, j * n_a + i)} if anchored else set()
            for s, di, dj in parts:
                if 0 <= i + di < n_a and 0 <= j + dj < n_b:
                    got.add((s, (j + dj) * n_a + i + di))
            want[j * n_a + i] = got
    return want


class RingState:
    """headers: 16 x [ia0, jb0, h0 bits, seq] as Python integers (the anchors signed); the frame's corner as the two floats of
    the step and its h0 bits; and, stated by hand: anchored, restart, v, q, parts = [(slot, di, dj)] in slot order."""

    def __init__(self, name, depth, n_a, n_b, headers, corner, h0, v, q, parts, restart=False, anchored=True, cell=1.0, note=""):
        assert len(headers) == 16
        self.name, self.depth, self.n_a, self.n_b, self.headers, self.corner, self.h0 = name, depth, n_a, n_b, headers, corner, h0
        self.v, self.q, self.parts, self.restart, self.anchored, self.cell, self.note = v, q, parts, restart, anchored, cell, note

    def step(self):
        w = gref.step_words(rcases.EYE, rcases.ZERO, [self.corner[0], self.corner[1], 0.0])
        w[14] = self.h0                                              # (the bits as they are: a NaN keeps its payload)
        return w

    def ground(self):
        return dict(JUDGE, n_a=self.n_a, n_b=self.n_b, cell_size=self.cell, quantum=sfc.QUANTUM, min_count=1, max_spread_q2=625)

    def frame(self, kind):
        n = self.n_a * self.n_b
        count, planes = signature(kind, n, FRAME_ENTRY)
        if kind == "relief":
            return count, planes[0].view(np.int64).copy(), planes[1].copy(), planes[2:].reshape(-1).view(np.int64).copy()
        return count, planes[0].view(np.int64).copy(), planes[1].copy()

    def render(self, kind):
        """-> the state block's bytes: the headers, then every slot's table holding its signature (an empty slot's too: stale)."""
        n = self.n_a * self.n_b
        slot = (rref if kind == "relief" else tref).slot_bytes(n)
        state = np.zeros(256 + self.depth * slot, dtype=np.uint8)
        state[:256].view(np.uint32).reshape(16, 4)[:] = np.array([[x & M32 for x in h] for h in self.headers], dtype=np.uint64).astype(np.uint32)
        for s in range(self.depth):
            count, planes = signature(kind, n, s)
            base = 256 + s * slot
            state[base:base + 8 * len(planes) * n].view(np.uint64)[:] = planes.reshape(-1)
            state[base + 8 * len(planes) * n:base + (8 * len(planes) + 4) * n].view(np.uint32)[:] = count
        return state

    def headers_after(self):
        """The 16 headers after the update, by hand."""
        h = [list(x) for x in self.headers]
        if not self.anchored:
            return h
        if self.restart:
            for s in range(self.depth):
                h[s] = [0, 0, 0, 0]
        h[self.v] = [int(np.rint(F32(self.corner[0]) * F32(1.0 / self.cell))), int(np.rint(F32(self.corner[1]) * F32(1.0 / self.cell))), self.h0, self.q]
        return h

    def status(self):
        if not self.anchored:
            return [max(h[3] for h in self.headers[:self.depth]), 0, 0, 0]
        after = self.headers_after()[self.v]
        return [self.q, len(self.parts) + 1, after[0] & M32, after[1] & M32]


def check_state(kind, st, got_count, got_planes, status, state_after, what):
    """What both the CPU and the GPU tests ask of an update from a planted state."""
    n = st.n_a * st.n_b
    want = hand_window(st.n_a, st.n_b, st.parts, st.anchored)
    for cell in range(n):
        got = decode(kind, got_count, got_planes, cell, what)
        for slot, src in sorted(got ^ want[cell]):
            raise AssertionError("%s: window cell %d: slot %d's entry of cell %d was %s" % (what, cell, slot, src, "added" if (slot, src) in got else "not added"))
    if kind == "relief":
        assert all(np.array_equal(got_planes[p + 4], got_planes[p]) for p in range(4)), "%s: planes 4 .. 7 repeat planes 0 .. 3" % what
        plane8 = [sum((src + 1) * (slot + 1) for slot, src in want[cell]) for cell in range(n)]
        assert [int(x) for x in got_planes[8]] == plane8, "%s: plane 8" % what
    assert [int(x) for x in status] == st.status(), "%s: status %s, by hand %s" % (what, list(status), st.status())
    assert not st.anchored or int(status[1]) == len(st.parts) + 1
    hdr = state_after[:256].view(np.uint32).reshape(16, 4)
    assert [[int(x) for x in h] for h in hdr] == [[x & M32 for x in h] for h in st.headers_after()], "%s: the headers after the update" % what
    before = st.render(kind)
    assert np.array_equal(hdr[st.depth:], before[:256].view(np.uint32).reshape(16, 4)[st.depth:]), "%s: headers beyond depth are untouched" % what
    slot = (len(before) - 256) // st.depth
    for s in range(st.depth):
        a, b = state_after[256 + s * slot:256 + (s + 1) * slot], before[256 + s * slot:256 + (s + 1) * slot]
        if st.anchored and s == st.v:
            count, planes = signature(kind, n, FRAME_ENTRY)
            assert np.array_equal(a[:8 * len(planes) * n].view(np.uint64), planes.reshape(-1)), "%s: slot v's table is the frame's" % what
            assert np.array_equal(a[8 * len(planes) * n:(8 * len(planes) + 4) * n].view(np.uint32), count), "%s: slot v's count is the frame's" % what
        else:
            assert np.array_equal(a, b), "%s: the table of slot %d was written" % (what, s)


IA0, JB0 = 100, -50
BASE_SEQ = [23, 9, 31, 12, 40, 17, 28, 11, 36, 14, 20, 33, 10, 26, 38, 19]          # the smallest at 1, the largest (40) at 4


def shifts16(n_a, n_b):
    """Sixteen different shifts in sight: zero, both signs, +-(n_a - 1) and +-(n_b - 1) alone and together."""
    return [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (2, -1), (-2, 1), (n_a - 1, 0), (-(n_a - 1), 0), (0, n_b - 1), (0, -(n_b - 1)),
            (n_a - 1, -(n_b - 1)), (-(n_a - 1), n_b - 1), (3, 2), (-3, -2), (1, 1)]


def hdr(di, dj, seq, h0=H_ONE):
    """The header of a slot whose table the frame at (IA0, JB0) reads at the shift (di, dj)."""
    return [IA0 - di, JB0 - dj, h0, seq]


def ring_states(n_a=6, n_b=5):
    """The depth-16 states on an n_a x n_b grid (n_a > n_b >= 4)."""
    sh = shifts16(n_a, n_b)
    corner = (float(IA0), float(JB0))
    out = []

    def add(name, seqs, v, q, takes, shifts=sh, h0s=None, frame_h0=H_ONE, restart=False, note=""):
        h0s = h0s or [H_ONE] * 16
        headers = [hdr(shifts[s][0], shifts[s][1], seqs[s], h0s[s]) for s in range(16)]
        parts = [(s, shifts[s][0], shifts[s][1]) for s in takes]
        out.append(RingState(name, 16, n_a, n_b, headers, corner, frame_h0, v, q, parts, restart=restart, note=note))

    others = lambda v: [s for s in range(16) if s != v]
    for at in (0, 7, 15):
        seqs = list(BASE_SEQ)
        seqs[1], seqs[at] = seqs[at], seqs[1]
        add("smallest_at_%d" % at, seqs, at, 41, others(at), note="the smallest seq, 9, at index %d, the rest in no order" % at)
    seqs = list(BASE_SEQ)
    seqs[9] = seqs[4] = 5
    add("tie_of_two", seqs, 4, 39, others(4), note="slots 9 and 4 tie at the smallest seq: 4 is replaced, 9 takes part")
    seqs = list(BASE_SEQ)
    for s in (12, 3, 8, 14, 6):
        seqs[s] = 5
    add("tie_of_five", seqs, 3, 41, others(3), note="five slots tie: the lowest index, 3, is replaced")
    big = [0x80000000, 0x7FFFFFFF, 0xFFFFFFFD, 0x80000001, 0x90000000, 0x7FFFFFFE, 0xC0000000, 0xFFFFFFFC, 0x80000002, 0xA0000000, 0xB0000000,
           0xD0000000, 0xE0000000, 0xF0000000, 0x8FFFFFFF, 0x9FFFFFFF]
    add("large_seqs", big, 5, 0xFFFFFFFE, others(5), note="seqs about 2^31 and up to 0xFFFFFFFD: unsigned, 0x7FFFFFFE at 5 is the smallest")
    seqs = list(BASE_SEQ)
    seqs[2] = 0xFFFFFFFE
    add("seq_fffffffe", seqs, 1, 0xFFFFFFFF, others(1), note="the largest seq is 0xFFFFFFFE: q is 0xFFFFFFFF, no restart yet")
    seqs[2] = 0xFFFFFFFF
    add("seq_ffffffff", seqs, 0, 1, [], restart=True, note="the largest seq is 0xFFFFFFFF: every slot is first taken as empty")
    add("fifteen_take_part", list(BASE_SEQ), 1, 41, others(1), note="fifteen participants, each at a shift of its own")
    # the edge of sight: +-(n - 1) is in sight by one row or column, +-n is not
    edge = [(n_a - 1, 0), (-(n_a - 1), 0), (0, n_b - 1), (0, -(n_b - 1)), (n_a, 0), (-n_a, 0), (0, n_b), (0, -n_b), (n_a, n_b - 1), (n_a - 1, n_b),
            (-n_a, -(n_b - 1)), (0, 0), (n_a - 1, n_b - 1), (-(n_a - 1), -(n_b - 1)), (1, -1), (-(n_a - 1), -n_b)]
    seqs = list(BASE_SEQ)
    seqs[1], seqs[14] = seqs[14], seqs[1]
    add("edge_of_sight", seqs, 14, 41, [0, 1, 2, 3, 11, 12, 13], shifts=edge, note="+-(n - 1) takes part, +-n does not")
    for name, shift in (("out_at_plus_n_a", (n_a, 0)), ("out_at_minus_n_a", (-n_a, 0)), ("out_at_plus_n_b", (0, n_b)), ("out_at_minus_n_b", (0, -n_b))):
        one = list(sh)
        one[6] = shift
        add(name, list(BASE_SEQ), 1, 41, [s for s in others(1) if s != 6], shifts=one, note="slot 6 alone lies exactly %s away" % (shift,))
    # holes: the frame's h0 is +0.0; a slot takes part with +0.0 or -0.0
    h0s = [H_PZERO, H_MZERO] * 8
    seqs = [0, 7, 0, 8, 5, 9, 6, 10, 0, 11, 12, 13, 14, 15, 16, 17]
    h0s[4], h0s[6] = H_ONE, H_NAN                                      # another h0; a NaN
    alt = list(sh)
    alt[10], alt[12], alt[14] = (0, -n_b), (n_a, 0), (-n_a, n_b)       # out of sight
    add("holes_alternating", seqs, 0, 18, [1, 3, 5, 7, 9, 11, 13, 15], shifts=alt, h0s=h0s, frame_h0=H_PZERO,
        note="the odd slots take part (-0.0 equals +0.0); the even ones are empty with stale tables (0, 2, 8), hold 1.0 (4) or a NaN (6), or lie out of sight (10, 12, 14)")
    seqs = [0, 0, 0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15]
    h0s = [H_ONE] * 3 + [H_TWO, H_MZERO, H_NAN] * 4 + [H_ONE]
    add("holes_only_the_last", seqs, 0, 16, [15], h0s=h0s, note="slot 15 alone: 0 .. 2 are empty, the rest hold another h0")
    seqs = [9, 3, 0, 0, 14, 5, 6, 7, 8, 2, 10, 11, 12, 13, 4, 15]
    h0s = [H_ONE] * 4 + [H_TWO] * 12
    add("holes_only_the_first", seqs, 2, 16, [0], h0s=h0s, note="slot 0 alone; 1 holds seq 3 but lies out of sight; 2 (replaced) and 3 are empty",
        shifts=[sh[0], (n_a, n_b)] + sh[2:])
    add("holes_none_nan", list(BASE_SEQ), 1, 41, [], h0s=[H_NAN] * 16, frame_h0=H_NAN, note="every h0 has the frame's NaN bits: a NaN matches nothing")
    add("all_but_slot_1", list(BASE_SEQ), 1, 41, others(1), shifts=[sh[1], sh[0]] + sh[2:],
        note="the replaced slot 1 holds the frame's h0, a shift of (0, 0) and a loud table: it is not added, its table is overwritten")
    # extreme anchors: the difference needs more than 32 bits
    for name, sign in (("extreme_anchors_low", -1), ("extreme_anchors_high", 1)):
        a0 = sign * (1 << 29)
        headers = [[INT32_MIN, INT32_MAX, H_ONE, 5], [INT32_MAX, INT32_MIN, H_ONE, 6], [-a0, a0, H_ONE, 7], [a0 + 1, -a0 - 2, H_ONE, 8], [-a0, -a0, H_ONE, 9],
                   [a0, a0, H_ONE, 10], [INT32_MIN, -a0, H_ONE, 11], [a0, INT32_MAX, H_ONE, 12]] + [[a0, -a0, H_ONE, 0]] * 8
        out.append(RingState(name, 16, n_a, n_b, headers, (float(a0), float(-a0)), H_ONE, 8, 13, [(3, -1, 2)],
                             note="stored anchors of INT32_MIN, INT32_MAX and -+2^29 against a frame at +-2^29: only slot 3, a cell away, is in sight"))
    return out


def depth_states():
    """The full list at depth 2 and 9 (7 x 4), and the headers beyond depth 3 (6 x 5)."""
    out = []
    sh = shifts16(7, 4)
    corner = (float(IA0), float(JB0))
    out.append(RingState("depth_2_full", 2, 7, 4, [hdr(0, 0, 4), hdr(6, -3, 9)] + [[0, 0, 0, 0]] * 14, corner, H_ONE, 0, 10, [(1, 6, -3)],
                         note="part_n == depth - 1 == 1"))
    seqs = [6, 7, 8, 3, 9, 10, 11, 12, 13]
    out.append(RingState("depth_9_full", 9, 7, 4, [hdr(sh[s + 5][0], sh[s + 5][1], seqs[s]) for s in range(9)] + [[0, 0, 0, 0]] * 7, corner, H_ONE, 3, 14,
                         [(s, sh[s + 5][0], sh[s + 5][1]) for s in range(9) if s != 3], note="part_n == depth - 1 == 8"))
    # headers beyond depth: a seq of 1 (smaller than any inside), of 0xFFFFFFFF (a restart if it were read), the frame's h0, in sight
    loud = [[IA0 - 1, JB0, H_ONE, 1 if s % 2 else 0xFFFFFFFF] for s in range(3, 16)]
    inside = [hdr(1, 0, 5), hdr(0, 1, 3), hdr(-1, -1, 4)]
    out.append(RingState("beyond_depth_update", 3, 6, 5, inside + loud, corner, H_ONE, 1, 6, [(0, 1, 0), (2, -1, -1)], note="headers 3 .. 15 are loud and ignored"))
    inside = [hdr(1, 0, 5), hdr(0, 1, 3), hdr(-1, -1, 0xFFFFFFFF)]
    out.append(RingState("beyond_depth_restart", 3, 6, 5, inside + loud, corner, H_ONE, 0, 1, [], restart=True, note="a restart zeroes headers 1 and 2 only"))
    inside = [hdr(1, 0, 5), hdr(0, 1, 3), hdr(-1, -1, 4)]
    out.append(RingState("beyond_depth_unanchored", 3, 6, 5, inside + loud, (float("nan"), float(JB0)), H_ONE, None, None, [], anchored=False,
                         note="a frame that is not anchored: status[0] is 5, the largest seq INSIDE the depth"))
    return out


def all_ring_states():
    return ring_states() + depth_states()


# ------------------------------------------------------------------------------------------------ (c) the ring, with its operators
def float_eq(a, b):
    return bool(np.array([a], dtype=np.uint32).view(F32)[0] == np.array([b], dtype=np.uint32).view(F32)[0])


def unsigned(x):
    return x & M32


def signed32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


RING_OPS = dict(anchor=operator.le, lo_a=operator.gt, hi_a=operator.lt, lo_b=operator.gt, hi_b=operator.lt, di_sign=1, swap=False, tie=operator.lt,
                seq_key=unsigned, nonzero=True, not_v=True, h0_eq=float_eq, restart=lambda largest: largest == M32, q=lambda largest: largest + 1,
                wide=lambda d: d)
RING_MUTATIONS = {
    "anchor < for <=": dict(anchor=operator.lt),
    "di > -n_a: >= for >": dict(lo_a=operator.ge),
    "di < n_a: <= for <": dict(hi_a=operator.le),
    "dj > -n_b: >= for >": dict(lo_b=operator.ge),
    "dj < n_b: <= for <": dict(hi_b=operator.le),
    "ia0 - h.x negated": dict(di_sign=-1),
    "di and dj exchanged": dict(swap=True),
    "the highest index on a tie": dict(tie=operator.le),
    "signed compare of seq": dict(seq_key=signed32),
    "seq != 0 dropped": dict(nonzero=False),
    "slot != v dropped": dict(not_v=False),
    "h0 compared as bits": dict(h0_eq=operator.eq),
    "restart at largest >= 0xFFFFFFFE": dict(restart=lambda largest: largest >= 0xFFFFFFFE),
    "q = largest without + 1": dict(q=lambda largest: largest),
    "32-bit wrap of di": dict(wide=signed32),
}


def ring_copy(headers, depth, n_a, n_b, corner, h0, inv_c=1.0, ops=None):
    """Steps 1, 3, 4 and 6 of the TERRAIN block for the 16 headers ([ia0, jb0, h0 bits, seq], Python integers) and a frame whose
    step holds the corner (two floats) and the bits of h0, its decisions taken from `ops` -> dict(anchored, restart, v, q,
    parts [(slot, di, dj)], status, headers: the 16 after the update).  With RING_OPS it is the specification."""
    op = dict(RING_OPS, **(ops or {}))
    with np.errstate(all="ignore"):
        ua, ub = F32(F32(corner[0]) * F32(inv_c)), F32(F32(corner[1]) * F32(inv_c))
        anchored = bool(op["anchor"](np.abs(ua), tref.ANCHOR_MAX)) and bool(op["anchor"](np.abs(ub), tref.ANCHOR_MAX))
    key = op["seq_key"]
    largest = max((h[3] for h in headers[:depth]), key=key) & M32
    after = [list(h) for h in headers]
    if not anchored:
        return dict(anchored=False, restart=False, v=None, q=None, parts=[], status=[largest, 0, 0, 0], headers=after)
    ia0, jb0 = int(np.rint(ua)), int(np.rint(ub))
    restart = bool(op["restart"](largest))
    v, parts = 0, []
    if restart:
        q = 1
        for s in range(depth):
            after[s] = [0, 0, 0, 0]
    else:
        q = op["q"](largest) & M32
        for s in range(1, depth):
            if op["tie"](key(headers[s][3]), key(headers[v][3])):
                v = s
        for s in range(depth):
            x, y, z, seq = headers[s]
            if (op["not_v"] and s == v) or (op["nonzero"] and seq & M32 == 0) or not op["h0_eq"](z & M32, h0 & M32):
                continue
            di, dj = op["wide"](op["di_sign"] * (ia0 - signed32(x))), op["wide"](jb0 - signed32(y))
            if op["swap"]:
                di, dj = dj, di
            if op["lo_a"](di, -n_a) and op["hi_a"](di, n_a) and op["lo_b"](dj, -n_b) and op["hi_b"](dj, n_b):
                parts.append((s, di, dj))
    after[v] = [ia0, jb0, h0 & M32, q]
    return dict(anchored=True, restart=restart, v=v, q=q, parts=parts, status=[q, len(parts) + 1, ia0 & M32, jb0 & M32], headers=after)


def random_state(rng):
    """A planted state at random: seqs with ties, zeros and large values, shifts about the edge of sight, h0 from a pool of five."""
    n_a, n_b = [(6, 5), (7, 4), (2, 2), (5, 3)][int(rng.integers(0, 4))]
    depth = int(rng.integers(1, 17))
    pool = [0, 0, 1, 2, 3, 3, 5, 5, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFD, 0xFFFFFFFE] + ([0xFFFFFFFF] if rng.random() < 0.1 else [])
    h0s = [H_ONE, H_ONE, H_ONE, H_TWO, H_PZERO, H_MZERO, H_NAN]
    headers = [[IA0 - int(rng.integers(-n_a - 1, n_a + 2)), JB0 - int(rng.integers(-n_b - 1, n_b + 2)), h0s[int(rng.integers(0, 7))],
                pool[int(rng.integers(0, len(pool)))]] for _ in range(16)]
    corner = (float(IA0), float(JB0)) if rng.random() < 0.95 else (float("inf"), 0.0)
    r = ring_copy(headers, depth, n_a, n_b, corner, h0s[int(rng.integers(0, 7))])
    return RingState("random", depth, n_a, n_b, headers, corner, r["headers"][r["v"]][2] if r["anchored"] else H_ONE, r["v"], r["q"], r["parts"],
                     restart=r["restart"], anchored=r["anchored"])


# ------------------------------------------------------------------------------------------------ (d) the terrain's cell formula
def by_hand(heights, min_count, max_spread_q2):
    """[(height, how many)] -> dict(count, sum, mean_q, S, spread_q2, flat): the GROUND block's cell in exact integers, S summed
    directly."""
    n, total = sum(c for _, c in heights), sum(h * c for h, c in heights)
    if n == 0:
        return dict(count=0, sum=0, mean_q=-(1 << 31), S=0, spread_q2=0xFFFFFFFF, flat=0)
    m = total // n
    S = sum((h - m) ** 2 * c for h, c in heights)
    return dict(count=n, sum=total, mean_q=m, S=S, spread_q2=S // n, flat=int(n >= min_count and S // n <= max_spread_q2))


class TerrainEdge:
    """Frames of integer heights, (corner, {world cell: [(height, how many)]}), for a terrain session of `depth`; `expect`:
    {update: {world cell: the outputs stated for it}}, the cell's part of it worked out by by_hand from the frames alone."""

    def __init__(self, name, edge, depth, frames, cfg, watch, sites=None, n_a=6, n_b=5):
        self.name, self.edge, self.depth, self.frames, self.cfg, self.n_a, self.n_b = name, edge, depth, frames, cfg, n_a, n_b
        self.expect = {}
        for t in range(len(frames)):
            for cell in watch:
                seen = [f for f in range(max(0, t - depth + 1), t + 1) if self.index(f, cell) is not None]
                assert t in seen
                heights = [hc for f in seen for hc in frames[f][1].get(cell, [])]
                self.expect.setdefault(t, {})[cell] = by_hand(heights, cfg["min_count"], cfg["max_spread_q2"])
        for (t, cell), site in (sites or {}).items():
            self.expect[t][cell]["site"] = site

    def ground(self):
        return dict(JUDGE, n_a=self.n_a, n_b=self.n_b, cell_size=sfc.CELL_SIZE, quantum=sfc.QUANTUM, **self.cfg)

    def index(self, f, cell):
        i, j = cell[0] - self.frames[f][0][0], cell[1] - self.frames[f][0][1]
        return j * self.n_a + i if 0 <= i < self.n_a and 0 <= j < self.n_b else None

    def frame(self, f):
        """-> (the step's words, (count uint32, sum int64, sum2 uint64)) as a ground call would have written them."""
        n = self.n_a * self.n_b
        count, total, total2 = [0] * n, [0] * n, [0] * n
        for cell, heights in self.frames[f][1].items():
            c = self.index(f, cell)
            if c is not None:
                count[c], total[c], total2[c] = sum(k for _, k in heights), sum(h * k for h, k in heights), sum(h * h * k for h, k in heights)
        assert max(count) < 1 << 32 and all(abs(h) <= gref.MAX_K for hs in self.frames[f][1].values() for h, _ in hs)
        return (rcases.corner_step(*self.frames[f][0]), (np.array(count, dtype=np.uint64).astype(np.uint32), np.array(total, dtype=np.int64),
                                                         np.array(total2, dtype=np.uint64)))


W0 = (102, -48)                                  # the watched world cell: grid cell (2, 2) from the corner (100, -50)
WALK = [(0, 0), (1, -1), (-1, 1), (1, 1), (-1, -1), (0, 1), (1, 0), (0, -1), (-1, 0)]      # the corners' offsets: W0 stays inside 6 x 5


def walk(f):
    return (100 + WALK[f % 9][0], -50 + WALK[f % 9][1])


def ones(*hs):
    return [(h, 1) for h in hs]


def terrain_edges():
    out = []
    plain_cfg = dict(min_count=1, max_spread_q2=625, max_step_q=40, window=0)
    frames = [(walk(f), {W0: ones(*hs)}) for f, hs in enumerate([(10, 12), (11, 9), (10, 10), (10,)])]
    out.append(TerrainEdge("min_count_by_the_window", "count 2, 4, 6 == min_count (flat), then 5 after an eviction", 3, frames, dict(plain_cfg, min_count=6), [W0]))
    # spread_q2 == max_spread_q2 and max_spread_q2 + 1: the last frame's two heights are the first pair, in a fixed order, that give 626
    base = [(25, 1), (-25, 1)]
    pair = next((a, b) for a in range(-60, 61) for b in range(a, 61) if by_hand(base * 2 + ones(a, b), 1, 625)["spread_q2"] == 626)
    frames = [(walk(f + 2), {W0: hs}) for f, hs in enumerate([base, base, base, ones(*pair)])]
    out.append(TerrainEdge("spread_at_and_above_the_bound", "spread_q2 625 == max_spread_q2 at update 2, 626 at update 3", 3, frames, plain_cfg, [W0]))
    frames = [(walk(f + 4), {W0: ones(*hs)}) for f, hs in enumerate([(-32767,), (-32766,), (-32767, 32767), (-32766, -32765, 3)])]
    out.append(TerrainEdge("floor_mean_of_a_negative_sum", "sums of -65,533 over 2 and over 4, and one more: the floor mean is not the truncated one", 3, frames,
                           dict(plain_cfg, max_spread_q2=0xFFFFFFFE), [W0]))
    # two neighbours a step apart, window 1: every cell of every frame holds one height 0, W0 holds 39, 40, 41, then 43 and 37
    nb = (W0[0] + 1, W0[1])
    frames = []
    for f, h in enumerate((39, 40, 41, 43, 37)):
        ia, jb = walk(f + 1)
        cells = {(ia + i, jb + j): ones(0) for j in range(5) for i in range(6)}
        cells[W0] = ones(h)
        frames.append(((ia, jb), cells))
    sites = {(2, W0): 1, (2, nb): 1, (3, W0): 0, (3, nb): 0, (4, W0): 1, (4, nb): 1}
    out.append(TerrainEdge("step_at_and_above_the_bound", "the window's means differ by 40 == max_step_q, by 41, and by 40 again: the sites go and return", 3,
                           frames, dict(plain_cfg, window=1), [W0, nb], sites=sites))
    # the largest window: 16 frames of 268,435,455 heights a cell, half of them 2 quanta apart, near +-32,767
    hi, lo = 134217728, 134217727
    frames = [(walk(f), {W0: [(32767, hi), (32765, lo)], nb: [(-32765, hi), (-32767, lo)]}) for f in range(16)]
    out.append(TerrainEdge("largest_window", "4,294,967,280 heights in a cell: the terms of S wrap modulo 2^64, S itself is the count and spread_q2 is 1", 16,
                           frames, plain_cfg, [W0, nb]))
    return out


def check_edge(e, outs, what=""):
    """The stated integers, cell by cell and update by update, in the outputs `outs` (the reference's or the device's)."""
    for t, cells in e.expect.items():
        for cell, want in cells.items():
            c = e.index(t, cell)
            for o, v in want.items():
                if o != "S":
                    assert int(outs[t][o][c]) == v, "%s %s, update %d, world cell %s: %s is %d, by hand %d" % (what, e.name, t, cell, o, int(outs[t][o][c]), v)


# ------------------------------------------------------------------------------------------------ (a) the pairs, located
def located_pairs(fam=None):
    """eviction_pairs -> [(session, sequence, track index, update t, before, after, what)]: the window is `before` at update t - 1
    and `after` at update t of that track."""
    out = []
    for before, after, what in eviction_pairs():
        for ss in all_sessions().values():
            for s in ss:
                for seq in s.sequences:
                    for b, tr in enumerate(seq.tracks):
                        held = tr.unnamed if before is None else tr.at.get(before, [])
                        ts = [u for u in tr.at.get(after, []) if u - 1 in held]
                        if ts and (fam is None or s.fam == fam):
                            out.append((s, seq, b, ts[0], before, after, what))
    return out
