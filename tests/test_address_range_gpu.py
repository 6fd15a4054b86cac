"""The device entry points of include/d2pc.h on frames placed beyond 2 and 4 GiB (tests/address_patterns.py).

The rest of the suite pins WHAT the kernels compute; this file varies WHERE the data lies and asserts that nothing else
changes.  Every case: the arenas hold a sentinel byte; small random frames (distinct per frame) are written into the
layout's views; the entry point runs on raw pointers; then

  1. every output region is byte-equal to the SAME context's output for the same frames in the dense layout;
  2. with the output regions copied out and refilled, every arena is all sentinel again: nothing else was written;
  3. the inputs are unchanged;
  4. one dense case per entry point is also held to the oracle, so that the file stands on its own.

One plane at a time lies in a big arena (`far16` / `far1`: frame 1 wholly above 4 GiB; `straddle`: offset 2^32 inside
frame 1; `tall`: rows either side of 4 GiB in one frame; `high`: the frame on the host's 32-bit limit, its last rows
above 2^31), the others are dense.  What each layout reaches and which slip it kills is asserted on the CPU in
tests/test_address_patterns.py; `Placed` refuses a layout that is not in address_patterns.gpu_geometries().
A kernel with one of the modelled slips FAILS here by comparison, it does not fault: every slipped byte lies inside the
arena."""
from types import SimpleNamespace

import numpy as np
import pytest

import address_patterns as ap
import colorize_ref
import disparity_to_point_cloud_amd as d2pc
import oracle
import score_filter_ref
from disparity_to_point_cloud_amd import capi
from helpers import assert_points_close, variant_for

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda"
S64 = int(np.array([ap.SENTINEL] * 8, dtype=np.uint8).view(np.int64)[0])
SMALL = 96 << 20
KNOWN = {L for _, L in ap.gpu_geometries()}
BIG = max(L.arena_bytes for s, L in ap.gpu_geometries() if "index plane" not in s)
INDEX_BASE = 9 << 29   # 4.5 GiB: where the index plane lives in the output arena when the points are laid out `far`
assert BIG <= int(6.5 * (1 << 30))


class Arena:
    def __init__(self, nbytes):
        self.t = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        self.t.fill_(ap.SENTINEL)

    def view(self, L):
        return self.t.as_strided((L.n_frames, L.rows, L.row_bytes), (max(L.frame_stride, 1), L.pitch, 1), L.base)

    def ptr(self, L):
        return self.t.data_ptr() + L.base

    def dirty(self):
        """A device flag: does any byte differ from the sentinel?  In chunks of 1 GiB."""
        bad = torch.zeros((), dtype=torch.bool, device=DEV)
        for o in range(0, self.t.numel(), 1 << 30):
            c = self.t[o:o + (1 << 30)]
            bad |= (c.view(torch.int64) != S64).any() if c.numel() % 8 == 0 else (c != ap.SENTINEL).any()
        return bad


@pytest.fixture(scope="module")
def mem():
    m = SimpleNamespace(big_in=Arena(BIG), big_out=Arena(BIG), small_in=Arena(SMALL), small_out=Arena(SMALL))
    torch.cuda.reset_peak_memory_stats()
    yield m
    print("\npeak device memory of test_address_range_gpu.py: %.3f GiB" % (torch.cuda.max_memory_allocated() / 2**30))
    for k in list(vars(m)):
        delattr(m, k)
    del m
    torch.cuda.empty_cache()


class Placed:
    """The planes of one call: inputs written into their layouts, outputs reserved; finish() collects the outputs and
    checks that nothing else changed."""

    def __init__(self, mem):
        self.mem, self.ins, self.outs, self.top = mem, {}, {}, {"in": 0, "out": 0}

    def _arena(self, L, side, base):
        if L.name == "dense":
            top = (self.top[side] + 511) // 256 * 256   # a guard of at least 256 sentinel bytes between planes
            L = L._replace(base=top)
            self.top[side] = top + ap.extent(L)
            assert self.top[side] + 256 <= SMALL
            return getattr(self.mem, "small_" + side), L
        if base is not None:
            L = L._replace(base=base)
        else:
            assert L in KNOWN, "a layout tests/test_address_patterns.py does not vouch for: %r" % (L,)
        assert L.base + ap.extent(L) <= BIG
        return getattr(self.mem, "big_" + side), L

    def put(self, name, frames, L):
        """frames: (n, rows, row_bytes) uint8 numpy."""
        a, L = self._arena(L, "in", None)
        src = torch.from_numpy(np.ascontiguousarray(frames)).to(DEV)
        assert tuple(src.shape) == (L.n_frames, L.rows, L.row_bytes)
        a.view(L).copy_(src)
        self.ins[name] = (a, L, src)
        return self.plane(name)

    def out(self, name, L, base=None):
        a, L = self._arena(L, "out", base)
        self.outs[name] = (a, L)
        return self.plane(name)

    def plane(self, name):
        a, L = (self.ins.get(name) or self.outs.get(name))[:2]
        return SimpleNamespace(ptr=a.ptr(L), pitch=L.pitch, stride=L.frame_stride, L=L)

    def finish(self):
        torch.cuda.synchronize()
        res, same = {}, {}
        for name, (a, L) in self.outs.items():
            v = a.view(L)
            res[name] = v.clone(memory_format=torch.contiguous_format)   # (a copy even where the view is contiguous)
            v.fill_(ap.SENTINEL)
        for name, (a, L, src) in self.ins.items():
            v = a.view(L)
            same[name] = torch.equal(v, src)
            v.fill_(ap.SENTINEL)
        dirty = {k: bool(getattr(self.mem, k).dirty()) for k in ("big_in", "big_out", "small_in", "small_out")}
        for k, d in dirty.items():   # (put it right for the next test before failing this one)
            if d:
                getattr(self.mem, k).t.fill_(ap.SENTINEL)
        assert all(same.values()), "an input changed: %r" % same
        assert not any(dirty.values()), "bytes outside the planes of the call were written: %r" % dirty
        return res


def rnd(seed, *shape):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def stream():
    return torch.cuda.current_stream().cuda_stream


def same(res, base, what, names=None):
    for k in names or base:
        assert torch.equal(res[k], base[k]), "%s: `%s` differs from the dense layout's (%d bytes)" % (
            what, k, int((res[k] != base[k]).sum()))


def bad_size(fn):
    with pytest.raises(d2pc.D2pcError) as e:
        fn()
    assert e.value.status == 3, e.value   # D2PC_ERR_BAD_SIZE
    torch.cuda.synchronize()


def nothing_launched(mem):
    """After a refused call (whose inputs were written beforehand and are cleared here): no output byte changed."""
    mem.big_in.t.fill_(ap.SENTINEL), mem.small_in.t.fill_(ap.SENTINEL)
    for k in ("big_out", "small_out"):
        assert not bool(getattr(mem, k).dirty()), k


# ------------------------------------------------------------------------------------------------------------ contexts
_ctx = {}


def ctx_for(algo=0, mode=d2pc.MODE_PARITY, border=40):
    key = (algo, variant_for(algo))
    if key not in _ctx:
        _ctx[key] = d2pc.Context(q=d2pc.make_q(), mode=d2pc.MODE_COMPACT, compact_algo=algo, variant=key[1])
    c = _ctx[key]
    c.set_mode(mode)
    c.set_border(border)
    for k, v in (("median_algo", 0), ("callback_fused", 1), ("callback_fused_compact", 2), ("fuse_rows", 0), ("score_tile", 0)):
        c.set_tuning(k, v)
    return c


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()
    _dense.clear()


_dense = {}   # the dense layout's result per (entry point, parameters): computed once, shared, never changed


def dense_of(key, run):
    if key not in _dense:
        _dense[key] = run()
    return _dense[key]


# ===================================================================================================================
# d2pc_process_device
# ===================================================================================================================
NP_DT = {d2pc.DTYPE_F32: np.float32, d2pc.DTYPE_U8: np.uint8, d2pc.DTYPE_U16: np.uint16}
SCALE = {d2pc.DTYPE_F32: 1.0, d2pc.DTYPE_U8: 0.125, d2pc.DTYPE_U16: 1.0 / 64}


def disparities(seed, dtype, n, h, w, holes=0.3):
    """Random disparities, distinct per frame; `holes`: the share of zeros (W = 0: what COMPACT removes)."""
    rng = np.random.default_rng(seed)
    if dtype == d2pc.DTYPE_F32:
        d = rng.uniform(0.5, 128.0, size=(n, h, w)).astype(np.float32)
    else:
        d = rng.integers(1, 256 if dtype == d2pc.DTYPE_U8 else 65536, size=(n, h, w)).astype(NP_DT[dtype])
    d[rng.random((n, h, w)) < holes] = 0
    return d


def as_bytes(frames):
    n, h, w = frames.shape
    return frames.view(np.uint8).reshape(n, h, w * frames.itemsize)


def process_layouts(kind_in, kind_out, n, h, w, es, roi_n):
    hp = ap.HIGH_PROCESS
    Lin = ap.high(h, w * es, hp["row_stride"]) if kind_in == "high" else ap.make(kind_in, h, w * es, es, n)
    Lp = ap.points(kind_out, roi_n, n)
    Li = ap.points(kind_out, roi_n, n, rec=4, point_stride=Lp.frame_stride // 16)
    return Lin, Lp, Li


def run_process(ctx, mem, frames, dtype, kind_in, kind_out, want_index, entry="process", k=0):
    """d2pc_process_device (or d2pc_process_mono_device with window k) on the layouts -> {points, index, counts}."""
    n, h, w = frames.shape
    b = ctx.config().border
    roi_n = (w - 2 * b) * (h - 2 * b)
    Lin, Lp, Li = process_layouts(kind_in, kind_out, n, h, w, frames.itemsize, roi_n)
    P = Placed(mem)
    src = P.put("disp", as_bytes(frames), Lin)
    pts = P.out("points", Lp)
    idx = P.out("index", Li, None if kind_out == "dense" else INDEX_BASE) if want_index else None
    cnt = P.out("counts", ap.dense(1, 4 * n, 1))
    sp = Lp.frame_stride // 16
    if entry == "process":
        ctx.process_device(src.ptr, dtype, SCALE[dtype], w, h, Lin.pitch, Lin.frame_stride, n, pts.ptr,
                           idx.ptr if idx else None, sp, cnt.ptr, stream())
    else:
        ctx.process_mono_device(src.ptr, dtype, w, h, Lin.pitch, Lin.frame_stride, n, k, 0.125, pts.ptr,
                                idx.ptr if idx else None, sp, cnt.ptr, stream())
    res = P.finish()
    ctx.check_async_error()
    res["counts"] = res["counts"].view(-1).view(torch.int32).cpu().numpy().view(np.uint32)
    return res


def same_cloud(res, base, roi_n, parity, what):
    assert np.array_equal(res["counts"], base["counts"]), (what, res["counts"], base["counts"])
    for f, c in enumerate(base["counts"]):
        assert c == roi_n if parity else c < roi_n, (what, c)
        for k in ("points", "index"):
            if k in base:
                assert torch.equal(res[k][f, :c], base[k][f, :c]), "%s: %s of frame %d differ from the dense layout's" % (what, k, f)


PLACES = [("far16", "dense"), ("far1", "dense"), ("straddle", "dense"), ("dense", "far16"), ("dense", "straddle"),
          ("far1", "straddle")]
SMALL_W = {"far16": 204}   # 16-byte row loads need a ROI width that is a multiple of four: 124 x 51 instead of 123 x 51


def small_frames(dtype, kind_in, seed=5):
    w = SMALL_W.get(kind_in, 203)
    return disparities(seed + w, dtype, 2, 131, w)


def check_against_oracle(frames, dtype, res, compact):
    b, q = 40, d2pc.make_q()
    for f, fr in enumerate(frames):
        got_p = res["points"][f].cpu().numpy().view(np.float32)
        got_i = res["index"][f].cpu().numpy().view(np.uint32).reshape(-1)
        if compact:
            wp, wi = oracle.reproject_compact(fr, q, border=b, scale=SCALE[dtype])
        else:
            wp = oracle.reproject(fr, q, border=b, scale=SCALE[dtype])
            h, w = fr.shape
            v, u = np.mgrid[b:h - b, b:w - b]
            wi = (v * w + u).reshape(-1).astype(np.uint32)
        c = int(res["counts"][f])
        assert c == len(wi) and np.array_equal(got_i[:c], wi)
        # the default form and the oracle's are each within 1 ulp of the exact value (tests/test_reproject_range_gpu.py)
        assert_points_close(got_p[:c], wp, max_ulp=2, what="frame %d against the oracle" % f)


@pytest.mark.parametrize("kind_in,kind_out", PLACES)
@pytest.mark.parametrize("want_index", [True, False])
@pytest.mark.parametrize("dtype", [d2pc.DTYPE_F32, d2pc.DTYPE_U8, d2pc.DTYPE_U16])
def test_process_device_parity(mem, dtype, want_index, kind_in, kind_out):
    frames = small_frames(dtype, kind_in)
    ctx = ctx_for()
    roi_n = (frames.shape[2] - 80) * 51
    base = dense_of(("parity", dtype, want_index, frames.shape), lambda: run_process(ctx, mem, frames, dtype, "dense", "dense", want_index))
    if want_index and (kind_in, kind_out) == PLACES[0]:
        check_against_oracle(frames, dtype, base, False)
    res = run_process(ctx, mem, frames, dtype, kind_in, kind_out, want_index)
    same_cloud(res, base, roi_n, True, "PARITY %s -> %s" % (kind_in, kind_out))


@pytest.mark.parametrize("kind_in,kind_out", PLACES)
@pytest.mark.parametrize("algo", [0, 1, 2, 3, 4])
def test_process_device_compact(mem, algo, kind_in, kind_out):
    """Every compaction algorithm (4: the experiment build's chunked two-pass); the launch counters confirm that the
    single pass (2) and the resident blocks (3) served their calls -- the two-frame call of algo 3 is the resident one."""
    dtype = d2pc.DTYPE_F32
    frames = small_frames(dtype, kind_in, seed=9)
    ctx = ctx_for(algo, d2pc.MODE_COMPACT)
    roi_n = (frames.shape[2] - 80) * 51
    base = dense_of(("compact", algo, frames.shape), lambda: run_process(ctx, mem, frames, dtype, "dense", "dense", True))
    if (kind_in, kind_out) == PLACES[0]:
        check_against_oracle(frames, dtype, base, True)
    st0 = ctx.compact_stats()
    res = run_process(ctx, mem, frames, dtype, kind_in, kind_out, True)
    st = ctx.compact_stats()
    assert st["timeouts"] == st0["timeouts"]
    if algo in (2, 3):
        assert st["launches"] == st0["launches"] + 1 and st["twopass_fallbacks"] == st0["twopass_fallbacks"], (st0, st)
    elif algo in (1, 4):
        assert st["launches"] == st0["launches"], (st0, st)
    same_cloud(res, base, roi_n, False, "COMPACT algo %d %s -> %s" % (algo, kind_in, kind_out))


def high_frames():
    hp = ap.HIGH_PROCESS
    return disparities(77, d2pc.DTYPE_F32, 1, hp["height"], hp["width"])


@pytest.mark.parametrize("mode,algo", [(d2pc.MODE_PARITY, 0), (d2pc.MODE_COMPACT, 0), (d2pc.MODE_COMPACT, 1), (d2pc.MODE_COMPACT, 2),
                                       (d2pc.MODE_COMPACT, 4)])
def test_process_device_on_the_host_limit(mem, mode, algo):
    """`high`: 61,440 rows 65,532 bytes apart -- (rows + 4097) * stride just below 2^32, the last rows above 2^31 --
    981,760 points, compared on the device; the PARITY cloud also against the oracle."""
    frames = high_frames()
    ctx = ctx_for(algo, mode)
    parity = mode == d2pc.MODE_PARITY
    base = dense_of(("high", mode, algo), lambda: run_process(ctx, mem, frames, d2pc.DTYPE_F32, "dense", "dense", True))
    res = run_process(ctx, mem, frames, d2pc.DTYPE_F32, "high", "dense", True)
    same_cloud(res, base, 981760, parity, "high, mode %d algo %d" % (mode, algo))
    if parity:   # (the oracle takes a second for the whole frame: no need to sample)
        hp = ap.HIGH_PROCESS
        want = oracle.reproject(frames[0], d2pc.make_q(), border=40)
        assert_points_close(res["points"][0].cpu().numpy().view(np.float32), want, max_ulp=2, what="high against the oracle")
        idx = res["index"][0].cpu().numpy().view(np.uint32).reshape(-1, 16)
        v, u = np.mgrid[40:hp["height"] - 40, 40:56]
        assert np.array_equal(idx, (v * hp["width"] + u).astype(np.uint32))


def test_process_device_refuses_the_first_size_past_its_limit(mem):
    """make_geom: (height + 4097) * row_stride <= 2^32 - 1.  One element of stride more is D2PC_ERR_BAD_SIZE and launches
    nothing; so is the same stride with the rows that no longer fit."""
    hp = ap.HIGH_PROCESS
    ctx = ctx_for()
    P = Placed(mem)
    out = P.out("points", ap.dense(1, 4096, 1))
    Lin = ap.high(hp["height"], hp["width"] * 4, hp["row_stride"])
    p = mem.big_in.ptr(Lin)
    assert ap.geom_fits(96, hp["height"], hp["row_stride"], 0, 1, 4) and not ap.geom_fits(96, hp["height"], hp["row_stride"] + 4, 0, 1, 4)
    bad_size(lambda: ctx.process_device(p, d2pc.DTYPE_F32, 1.0, 96, hp["height"], hp["row_stride"] + 4, 0, 1, out.ptr, None, 0, None, stream()))
    rows = 0xFFFFFFFF // hp["row_stride"] - 4097 + 1
    assert ap.geom_fits(96, rows - 1, hp["row_stride"], 0, 1, 4) and not ap.geom_fits(96, rows, hp["row_stride"], 0, 1, 4)
    bad_size(lambda: ctx.process_device(p, d2pc.DTYPE_F32, 1.0, 96, rows, hp["row_stride"], 0, 1, out.ptr, None, 0, None, stream()))
    P.finish()


def test_index_plane_past_4_gib():
    """out_frame_stride_points = 2^30 + 16: frame 1 of the INDEX plane lies 2^32 + 64 bytes in (and frame 1 of the points
    16 GiB in).  PARITY and the default COMPACT.  The one test of this file that may skip: when the device cannot hold the
    16 GiB arena."""
    sp = ap.FAR_INDEX_POINT_STRIDE
    frames = small_frames(d2pc.DTYPE_F32, "dense", seed=21)
    n, h, w = frames.shape
    roi_n = 123 * 51
    Li = ap.points("far16", roi_n, rec=4, point_stride=sp)
    assert Li in KNOWN
    try:
        pts, idx = Arena(256 + sp * 16 + roi_n * 16 + 4096), Arena(Li.arena_bytes)
    except torch.cuda.OutOfMemoryError:
        pytest.skip("the device cannot hold the 16 GiB points arena")
    Lp = Li._replace(pitch=16, row_bytes=16, frame_stride=sp * 16, arena_bytes=pts.t.numel())
    src = torch.from_numpy(frames).to(DEV)
    cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
    for mode in (d2pc.MODE_PARITY, d2pc.MODE_COMPACT):
        ctx = ctx_for(0, mode)
        ctx.process_device(src.data_ptr(), d2pc.DTYPE_F32, 1.0, w, h, w * 4, w * h * 4, n, pts.ptr(Lp), idx.ptr(Li), sp, cnt.data_ptr(), stream())
        torch.cuda.synchronize()
        ctx.check_async_error()
        counts = cnt.cpu().numpy().view(np.uint32)
        got_p = pts.view(Lp).contiguous().cpu().numpy().view(np.float32)
        got_i = idx.view(Li).contiguous().cpu().numpy().view(np.uint32).reshape(n, roi_n)
        pts.view(Lp).fill_(ap.SENTINEL), idx.view(Li).fill_(ap.SENTINEL)
        assert not bool(pts.dirty()) and not bool(idx.dirty()), "mode %d: bytes outside the frames' points or indices were written" % mode
        for f in range(n):
            if mode == d2pc.MODE_PARITY:
                wp = oracle.reproject(frames[f], d2pc.make_q(), border=40)
                v, u = np.mgrid[40:h - 40, 40:w - 40]
                wi = (v * w + u).reshape(-1).astype(np.uint32)
            else:
                wp, wi = oracle.reproject_compact(frames[f], d2pc.make_q(), border=40)
            assert counts[f] == len(wi) and np.array_equal(got_i[f, :len(wi)], wi), (mode, f)
            assert_points_close(got_p[f, :len(wi)], wp, max_ulp=2, what="mode %d frame %d" % (mode, f))
    del pts, idx
    torch.cuda.empty_cache()


# ===================================================================================================================
# d2pc_process_mono_device
# ===================================================================================================================
MONO_FORMS = {"fused PARITY": (d2pc.MODE_PARITY, "callback_fused", 1), "fused COMPACT": (d2pc.MODE_COMPACT, "callback_fused_compact", 2),
              "two launches": (d2pc.MODE_PARITY, "callback_fused", 0), "two launches, COMPACT": (d2pc.MODE_COMPACT, "callback_fused_compact", 0)}


@pytest.mark.parametrize("kind_in,kind_out", [("far16", "dense"), ("far1", "dense"), ("straddle", "dense"), ("dense", "far16"), ("far1", "far16")])
@pytest.mark.parametrize("dtype", [d2pc.DTYPE_U8, d2pc.DTYPE_MONO16])
@pytest.mark.parametrize("form", list(MONO_FORMS))
def test_process_mono_device(mem, form, dtype, kind_in, kind_out):
    """The callback body as one kernel per tile (bit-sliced median, median_algo 2) and as two launches, 8-bit and mono16
    frames; the dense PARITY result against the oracle's rescale, median and reprojection."""
    mode, key, value = MONO_FORMS[form]
    rng = np.random.default_rng(31)
    smooth = (rng.integers(0, 40, size=(2, 131, 203)) + np.arange(203)[None, None, :] // 2 + 60 * np.arange(2)[:, None, None])
    frames = (smooth * 257 + rng.integers(0, 257, size=smooth.shape)).astype(np.uint16) if dtype == d2pc.DTYPE_MONO16 else smooth.astype(np.uint8)
    ctx = ctx_for(0, mode)

    def run(ki, ko):
        ctx.set_tuning("median_algo", 2)
        ctx.set_tuning(key, value)
        return run_process(ctx, mem, frames, dtype, ki, ko, True, entry="mono", k=11)
    base = dense_of(("mono", form, dtype), lambda: run("dense", "dense"))
    if (kind_in, kind_out) == ("far16", "dense"):
        for f in range(2):
            m8 = oracle.mono16_to_mono8(frames[f]) if dtype == d2pc.DTYPE_MONO16 else frames[f]
            filt = oracle.median_u8(m8, 11)
            if mode == d2pc.MODE_PARITY:
                want, c = oracle.reproject(filt, d2pc.make_q(), border=40, scale=0.125), 123 * 51
            else:
                want, wi = oracle.reproject_compact(filt, d2pc.make_q(), border=40, scale=0.125)
                c = len(wi)
                assert np.array_equal(base["index"][f].cpu().numpy().view(np.uint32).reshape(-1)[:c], wi)
            assert base["counts"][f] == c
            assert_points_close(base["points"][f].cpu().numpy().view(np.float32)[:c], want, max_ulp=2, what="%s frame %d" % (form, f))
    res = run(kind_in, kind_out)
    assert np.array_equal(res["counts"], base["counts"])
    for f, c in enumerate(base["counts"]):
        for k in ("points", "index"):
            assert torch.equal(res[k][f, :c], base[k][f, :c]), "%s %s -> %s: %s of frame %d" % (form, kind_in, kind_out, k, f)


# ===================================================================================================================
# image planes: one generic runner
# ===================================================================================================================
class Op:
    """One call of an image entry point: named input planes (numpy (n, rows, row_bytes) uint8), named output planes
    ((rows, row_bytes)), and `call(ctx, planes)` with planes[name] = (ptr, pitch, stride)."""

    def __init__(self, key, n, ins, outs, call, elem=None):
        self.key, self.n, self.ins, self.outs, self.call, self.elem = key, n, ins, outs, call, elem or {}

    def run(self, ctx, mem, exotic=None, kind="dense"):
        P, planes = Placed(mem), {}
        for name, fr in self.ins.items():
            k = kind if name == exotic else "dense"
            planes[name] = P.put(name, fr, ap.make(k, fr.shape[1], fr.shape[2], self.elem.get(name, 1), self.n))
        for name, (rows, rb) in self.outs.items():
            planes[name] = P.out(name, ap.make(kind if name == exotic else "dense", rows, rb, 1, self.n))
        self.call(ctx, planes)
        return P.finish()

    def check(self, ctx, mem, exotic, kind, want=None):
        """Dense once (against `want()`: {output: numpy (n, rows, row_bytes)}, where given), then the layout."""
        first = self.key not in _dense
        base = dense_of(self.key, lambda: self.run(ctx, mem))
        if first and want is not None:
            for name, w in want().items():
                assert np.array_equal(base[name].cpu().numpy(), w.reshape(base[name].shape)), "%s: dense `%s` against the oracle" % (self.key, name)
        same(self.run(ctx, mem, exotic, kind), base, "%s, `%s` on %s" % (self.key, exotic, kind))


def n_for(kind):
    return 1 if kind in ("tall", "high") else 2


# ------------------------------------------------------------------------------------------------------------- medians
def median_op(kind, k, algo, roi):
    n, (w, h) = n_for(kind), ((203, 70) if kind == "tall" else (203, 131))
    border = 8 if kind == "tall" else 40
    src = rnd(100 + h, n, h, w)

    def call(ctx, p):
        ctx.set_tuning("median_algo", algo)
        ctx.set_border(border)
        fn = ctx.median_roi_device if roi else ctx.median_device
        fn(p["src"].ptr, w, h, p["src"].pitch, p["src"].stride, n, p["dst"].ptr, p["dst"].pitch, p["dst"].stride, k, stream())

    def want():
        full = np.stack([oracle.median_u8(f, k) for f in src])
        if roi:
            out = np.full_like(full, ap.SENTINEL)
            out[:, border:h - border, border:w - border] = full[:, border:h - border, border:w - border]
            return {"dst": out}
        return {"dst": full}
    return Op(("median", n, h, k, algo, roi), n, {"src": src}, {"dst": (h, w)}, call), want


@pytest.mark.parametrize("kind", ["far16", "far1", "straddle", "tall"])
@pytest.mark.parametrize("exotic", ["src", "dst"])
@pytest.mark.parametrize("roi", [False, True])
@pytest.mark.parametrize("k,algo", [(11, 0), (11, 1), (11, 2), (3, 0), (5, 2)])
def test_median_devices(mem, k, algo, roi, exotic, kind):
    op, want = median_op(kind, k, algo, roi)
    op.check(ctx_for(), mem, exotic, kind, want)


@pytest.mark.parametrize("kind", ["far16", "far1", "straddle", "tall"])
@pytest.mark.parametrize("exotic", ["src", "dst"])
def test_mono16_to_mono8_device(mem, exotic, kind):
    n, (w, h) = n_for(kind), ((203, 70) if kind == "tall" else (203, 131))
    img = np.random.default_rng(h).integers(0, 65536, size=(n, h, w)).astype(np.uint16)

    def call(ctx, p):
        ctx.mono16_to_mono8_device(p["src"].ptr, w, h, p["src"].pitch, p["src"].stride, n, p["dst"].ptr, p["dst"].pitch, p["dst"].stride, stream())
    op = Op(("mono16", n, h), n, {"src": as_bytes(img)}, {"dst": (h, w)}, call, elem={"src": 2})
    op.check(ctx_for(), mem, exotic, kind, lambda: {"dst": np.stack([oracle.mono16_to_mono8(f) for f in img])})


# -------------------------------------------------------------------------------------------------------------- rotate
def frame_for(kind, exotic_is_rotated_output):
    """(cols, rows): 129 x 65 crosses a tile both ways; on `tall` the plane under test has 70 rows."""
    if kind != "tall":
        return 129, 65
    return (70, 129) if exotic_is_rotated_output else (129, 70)


@pytest.mark.parametrize("kind", ["far16", "far1", "straddle", "tall"])
@pytest.mark.parametrize("exotic", ["src", "dst"])
def test_rotate_cw_device(mem, exotic, kind):
    n, (cols, rows) = n_for(kind), frame_for(kind, exotic == "dst")
    src = rnd(cols, n, rows, cols)

    def call(ctx, p):
        ctx.rotate_cw_device(p["src"].ptr, cols, rows, p["src"].pitch, p["src"].stride, n, p["dst"].ptr, p["dst"].pitch, p["dst"].stride, stream())
    op = Op(("rotate", n, cols, rows), n, {"src": src}, {"dst": (cols, rows)}, call)
    op.check(ctx_for(), mem, exotic, kind, lambda: {"dst": np.stack([oracle.rotate_cw(f) for f in src])})


# ------------------------------------------------------------------------------------------------------------ colorize
@pytest.mark.parametrize("kind", ["far16", "far1", "straddle", "tall"])
@pytest.mark.parametrize("exotic", ["src", "gray", "rgb"])
@pytest.mark.parametrize("rotate", [0, 1])
def test_colorize_device(mem, rotate, exotic, kind):
    """The view and its colouring, of the frame and of the frame rotated; `far1` gives the rgb plane a base and a pitch
    that are not multiples of 4 (the spliced stores)."""
    n, (cols, rows) = n_for(kind), frame_for(kind, bool(rotate) and exotic != "src")
    fw, fh = (rows, cols) if rotate else (cols, rows)
    view = (0, 0, fw, fh) if kind == "tall" else (3, 2, fw - 5, fh - 3)
    x, y, w, h = view
    src = rnd(7 * cols + rotate, n, rows, cols)

    def call(ctx, p):
        d = d2pc.colorize_desc_init()
        d.rotate_cw, d.cols, d.rows, d.n_frames = rotate, cols, rows, n
        d.x, d.y, d.w, d.h = view
        d.src, d.src_pitch, d.src_frame_stride = p["src"].ptr, p["src"].pitch, p["src"].stride
        d.gray, d.gray_pitch, d.gray_frame_stride = p["gray"].ptr, p["gray"].pitch, p["gray"].stride
        d.rgb, d.rgb_pitch, d.rgb_frame_stride = p["rgb"].ptr, p["rgb"].pitch, p["rgb"].stride
        ctx.colorize_device(d, stream())

    def want():
        got = [colorize_ref.colorize_view(f, view, bool(rotate)) for f in src]
        return {"rgb": np.stack([g[0] for g in got]), "gray": np.stack([g[1] for g in got])}
    if exotic == "rgb" and kind == "far1":
        L = ap.make(kind, h, 3 * w, 1, n)
        assert L.base % 4 and L.pitch % 4
    op = Op(("colorize", n, cols, rows, rotate), n, {"src": src}, {"gray": (h, w), "rgb": (h, 3 * w)}, call)
    op.check(ctx_for(), mem, exotic, kind, want)


# ---------------------------------------------------------------------------------------------------------------- fuse
FUSE_IN = ("depth1", "depth2", "score1", "score2", "grad1", "grad2")
FUSE_CROP = (3, 5, 2, 1)


def fuse_op(kind, shape, rule, fuse_rows, pitch_step=0, row_step=0):
    n = n_for(kind)
    w, h = (61, ap.HIGH_PLANE_ROWS) if kind == "high" else shape
    l, r, t, b = FUSE_CROP
    ins = {name: rnd(11 * i + w, n, h, w) for i, name in enumerate(FUSE_IN)}
    for s in ("score1", "score2"):
        ins[s] = (ins[s] // 2).astype(np.uint8)   # (scores either side of the rules' thresholds)

    def call(ctx, p):
        ctx.set_tuning("fuse_rows", fuse_rows)
        d = d2pc.fuse_desc_init()
        d.rule, d.width, d.height, d.n_frames = rule, w, h + row_step, n
        d.crop_left, d.crop_right, d.crop_top, d.crop_bottom = FUSE_CROP
        for i, name in enumerate(FUSE_IN):
            d.planes[i], d.pitch[i], d.frame_stride[i] = p[name].ptr, p[name].pitch + (pitch_step if p[name].L.name == "high" else 0), p[name].stride
        for name in ("fused", "combined"):
            step = pitch_step if p[name].L.name == "high" else 0
            setattr(d, name, p[name].ptr), setattr(d, name + "_pitch", p[name].pitch + step), setattr(d, name + "_frame_stride", p[name].stride)
        ctx.fuse_device(d, stream())

    def want():
        got = [oracle.fuse([ins[k][f] for k in FUSE_IN], rule=rule, crop=FUSE_CROP) for f in range(n)]
        return {"fused": np.stack([g[0] for g in got]), "combined": np.stack([g[1] for g in got])}
    return Op(("fuse", n, w, h, rule, fuse_rows), n, ins, {"fused": (h - t - b, w - l - r), "combined": (h, w)}, call), want


@pytest.mark.parametrize("kind", ["far16", "far1", "straddle", "high"])
@pytest.mark.parametrize("exotic", FUSE_IN + ("fused", "combined"))
@pytest.mark.parametrize("rule,fuse_rows,shape", [(d2pc.FUSE_GRAD_FILTER, 0, (249, 9)), (d2pc.FUSE_GRAD_FILTER, 2, (61, 83)),
                                                   (d2pc.FUSE_BETTER_SCORE, 0, (61, 83)), (d2pc.FUSE_BETTER_SCORE, 2, (249, 9))])
def test_fuse_device(mem, rule, fuse_rows, shape, exotic, kind):
    op, want = fuse_op(kind, shape, rule, fuse_rows)
    op.check(ctx_for(), mem, exotic, kind, want)


@pytest.mark.parametrize("exotic", ["depth2", "grad1", "fused", "combined"])
@pytest.mark.parametrize("step", ["pitch", "row"])
def test_fuse_device_refuses_the_first_size_past_its_limit(mem, exotic, step):
    """Bound32::Plane: pitch * rows <= 2^32 - 1.  `high` is the largest pitch for its rows (the accepted call is
    test_fuse_device[high]); one byte of pitch more, or one row more, is D2PC_ERR_BAD_SIZE and launches nothing."""
    op, _ = fuse_op("high", None, d2pc.FUSE_GRAD_FILTER, 0, pitch_step=int(step == "pitch"), row_step=int(step == "row"))
    ctx = ctx_for()
    bad_size(lambda: op.run(ctx, mem, exotic, "high"))
    nothing_launched(mem)


# -------------------------------------------------------------------------------------------------------- score filter
def score_op(kind, exotic, nn, direction, form, tile, pitch_step=0, row_step=0):
    n = n_for(kind)
    if kind == "high" and exotic == "src":
        width, height, x, y = 80, ap.HIGH_PLANE_ROWS, 5, ap.HIGH_PLANE_ROWS - nn - 4   # the square sits in the rows above 2^31
    else:
        width, height, x, y = nn + 13, nn + 10, 6, 5
    rng = np.random.default_rng(nn + direction)
    src = (rng.integers(0, 120, size=(n, height, width)) + 90 * ((np.arange(width)[None, None, :] // 9 + np.arange(height)[None, :, None] // 7) % 2)).astype(np.uint8)

    def call(ctx, p):
        ctx.set_tuning("score_tile", tile)
        d = d2pc.score_filter_desc_init()
        d.direction, d.form, d.width, d.height, d.n_frames = direction, form, width, height + (row_step if exotic == "src" else 0), n
        d.x, d.y, d.n = x, y, nn + (row_step if exotic != "src" else 0)
        for name in ("src", "out", "grad"):
            step = pitch_step if p[name].L.name == "high" else 0
            setattr(d, name, p[name].ptr), setattr(d, name + "_pitch", p[name].pitch + step), setattr(d, name + "_frame_stride", p[name].stride)
        ctx.score_filter_device(d, stream())

    def want():
        got = [score_filter_ref.score_filter(f, (x, y, nn), direction, form) for f in src]
        return {"out": np.stack([g[0] for g in got]), "grad": np.stack([g[1] for g in got])}
    return Op(("score", n, width, height, nn, direction, form, tile), n, {"src": src}, {"out": (nn, nn), "grad": (nn, nn)}, call), want


@pytest.mark.parametrize("kind", ["far16", "far1", "straddle", "high"])
@pytest.mark.parametrize("exotic", ["src", "out", "grad"])
@pytest.mark.parametrize("nn,direction,form,tile", [(45, 0, 4, 32), (45, 1, 3, 64), (70, 1, 4, 32), (70, 0, 3, 64)])
def test_score_filter_device(mem, nn, direction, form, tile, exotic, kind):
    op, want = score_op(kind, exotic, nn, direction, form, tile)
    op.check(ctx_for(), mem, exotic, kind, want)


@pytest.mark.parametrize("exotic", ["src", "out", "grad"])
@pytest.mark.parametrize("step", ["pitch", "row"])
def test_score_filter_device_refuses_the_first_size_past_its_limit(mem, exotic, step):
    """As for the fusion: one byte of pitch, or one row (of the frame; of the square for `out` and `grad`), past `high`."""
    op, _ = score_op("high", exotic, 70, 0, 4, 0, pitch_step=int(step == "pitch"), row_step=int(step == "row"))
    ctx = ctx_for()
    bad_size(lambda: op.run(ctx, mem, exotic, "high"))
    nothing_launched(mem)


# ===================================================================================================================
# the fusion node's session
# ===================================================================================================================
NODE_CALLS = [(d2pc.NODE_MATCHING_SCORE_1, "matching_score_1"), (d2pc.NODE_MATCHING_SCORE_2, "matching_score_2"),
              (d2pc.NODE_DISPARITY_1, "disparity_1"), (d2pc.NODE_DISPARITY_2, "disparity_2")]


@pytest.mark.parametrize("kind", ["far16", "far1", "straddle", "tall"])
@pytest.mark.parametrize("single_launch", [1, 0])
def test_fusion_node_callback_device(mem, single_launch, kind):
    """The four callbacks on raw frames in the layout (a batch of 2; one frame of 70 rows on `tall`: camera 2's two
    callbacks and DISPARITY_1 take it, MATCHING_SCORE_1 refuses it), the last a fusing DISPARITY_2: every published
    topic against colorize_ref.RefNode, frame by frame."""
    batch = n_for(kind)
    cols, rows = (188, 70) if kind == "tall" else (188, 120)
    ctx = ctx_for()
    s = capi.FusionSession(ctx, cols, rows, batch=batch, single_launch=single_launch)
    models = [colorize_ref.RefNode(cols, rows) for _ in range(batch)]
    rng = np.random.default_rng(rows + single_launch)
    published = set()
    try:
        for i, (which, name) in enumerate(NODE_CALLS):
            fr = rng.integers(0, 256, size=(batch, rows, cols)).astype(np.uint8)
            if "score" in name:
                fr = (fr // 3 + 80 * ((np.arange(cols)[None, None, :] // 11) % 2)).astype(np.uint8)
            kind_i = kind
            if kind == "tall" and which == d2pc.NODE_MATCHING_SCORE_1:
                # camera 1's score frame goes to the score filter as it is, and that forms row offsets in 32 bits
                # (Bound32::Plane): the session refuses the frame, launches nothing and stays usable
                P = Placed(mem)
                p = P.put("frame", fr, ap.make(kind, rows, cols, 1, batch))
                bad_size(lambda: s.callback_device(which, p.ptr, p.pitch, p.stride, stream()))
                P.finish()
                kind_i = "dense"
            P = Placed(mem)
            p = P.put("frame", fr, ap.make(kind_i, rows, cols, 1, batch))
            views = s._views(s.callback_device(which, p.ptr, p.pitch, p.stride, stream()))
            torch.cuda.synchronize()
            got = {k: (v.cpu().numpy()[None] if batch == 1 else v.cpu().numpy()) for k, v in views.items()}
            P.finish()
            for f in range(batch):
                want = getattr(models[f], name)(fr[f])
                assert set(want) == set(got), (name, sorted(want), sorted(got))
                for topic, w in want.items():
                    assert np.array_equal(got[topic][f], w), "%s on %s: topic %s of pair %d" % (name, kind, topic, f)
                published |= set(want)
        assert {"cropped_depth_2", "combined_score", "gradient", "fused_depth_map"} <= published
    finally:
        s.close()
