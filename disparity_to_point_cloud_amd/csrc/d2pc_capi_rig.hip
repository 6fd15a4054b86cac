// d2pc_capi_rig.hip -- include/d2pc.h, the rig session (d2pc_rig_*): n cameras of one geometry, one Q each (a pose folded
// in as T.Q), one merged cloud per call.  The per-camera calibrations live in a device table the kernels of d2pc_rig.hip
// read; the tile counts of the COMPACT form are the rig's own, allocated once for border 0.  Planes are checked through
// d2pc_plane.hpp: the frames with Bound32::Plane (the kernels form a row's offset in 32 bits), FrameRule::LastRow.
// At the end: the textured clouds (d2pc_texture_*), which need no session -- here for the product library's size budget.
#include "d2pc_ctx.hpp"
#include "d2pc_rig.hpp"

using namespace d2pc;
using namespace d2pc::host;

static_assert(kRigMaxCameras == D2PC_RIG_MAX_CAMERAS, "the scan kernel's offsets live in LDS, one per camera");

struct d2pc_rig {
  d2pc_ctx *ctx = nullptr;
  d2pc_rig_config cfg{};
  std::vector<double> q;       // n x 16, as handed over
  RigCal *d_table = nullptr;   // n entries
  uint32_t *d_tiles = nullptr; // 4 words per tile of 256 * kRigCompactPxt pixels, every camera, border 0
};

namespace {

uint64_t tiles_of(uint64_t points, int pxt) {
  const uint64_t tile = uint64_t(kBlock) * uint64_t(pxt);
  return (points + tile - 1) / tile;
}

// what geometry, create and process refuse alike; roi = ROI points of one camera
int check(const d2pc_rig_config *c, int border, uint64_t *roi) {
  if (!c || c->struct_size != sizeof(d2pc_rig_config)) return D2PC_ERR_INVALID_ARG;
  if (c->n_cameras < 1 || c->n_cameras > D2PC_RIG_MAX_CAMERAS || border < 0 || border > 16384) return D2PC_ERR_INVALID_ARG;
  if (c->dtype != D2PC_DTYPE_F32 && c->dtype != D2PC_DTYPE_U8 && c->dtype != D2PC_DTYPE_U16) return D2PC_ERR_BAD_DTYPE;
  if (c->width <= 0 || c->height <= 0) return D2PC_ERR_BAD_SIZE;
  if (uint64_t(c->width) * uint64_t(c->height) > (uint64_t(1) << 31)) return D2PC_ERR_BAD_SIZE;
  *roi = d2pc_roi_points(c->width, c->height, border);
  if (*roi > (uint64_t(1) << 28)) return D2PC_ERR_BAD_SIZE;
  if (*roi * uint64_t(c->n_cameras) >= (uint64_t(1) << 32)) return D2PC_ERR_BAD_SIZE;  // a point's position is 32 bits
  return D2PC_OK;
}

bool index_available(const d2pc_rig_config &c) {
  return uint64_t(c.n_cameras) * uint64_t(c.width) * uint64_t(c.height) <= (uint64_t(1) << 32);
}

size_t tile_bytes(const d2pc_rig_config &c) {
  return size_t(tiles_of(uint64_t(c.width) * uint64_t(c.height), kRigCompactPxt)) * size_t(c.n_cameras) * 16u;
}

// one table entry: the constants as classify_q and fill_q form them for a context (d2pc_capi_context.hip)
void fill_entry(d2pc_ctx *scratch, const double q[16], RigCal *e) {
  memcpy(scratch->q, q, sizeof scratch->q);
  classify_q(scratch);
  memcpy(e->q, q, sizeof e->q);
  e->cx = scratch->qs.cx, e->cy = scratch->qs.cy, e->f = scratch->qs.f, e->a = scratch->qs.a, e->b = scratch->qs.b;
  e->f_cv4 = double(float(e->f));
  e->stereo = scratch->q_kind == QK_STEREO ? 1u : 0u;
  e->pad = 0;
}

struct QScratch {  // classify_q reads and writes a context's q, q_kind and qs only: a bare one serves
  d2pc_ctx *c = new (std::nothrow) d2pc_ctx();
  ~QScratch() { delete c; }
};

}  // namespace

extern "C" {

void d2pc_rig_config_init(d2pc_rig_config *cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = sizeof *cfg;
  cfg->n_cameras = 1;
  cfg->dtype = D2PC_DTYPE_F32;
}

int d2pc_rig_geometry(const d2pc_rig_config *cfg, int border, d2pc_rig_geometry_t *out) {
  if (!out) return D2PC_ERR_INVALID_ARG;
  uint64_t roi = 0;
  const int st = check(cfg, border, &roi);
  if (st != D2PC_OK) return st;
  memset(out, 0, sizeof *out);
  out->roi_points = size_t(roi);
  out->capacity_points = size_t(roi) * size_t(cfg->n_cameras);
  out->device_bytes = size_t(cfg->n_cameras) * sizeof(RigCal) + tile_bytes(*cfg);
  out->index_available = index_available(*cfg) ? 1 : 0;
  return D2PC_OK;
}

int d2pc_rig_compose_q(const double t[16], const double q[16], double out[16]) {
  if (!t || !q || !out) return D2PC_ERR_INVALID_ARG;
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(t[i]) || !std::isfinite(q[i])) return D2PC_ERR_INVALID_ARG;
  double r[16];
  {
#pragma clang fp contract(off)
    for (int i = 0; i < 4; ++i)
      for (int k = 0; k < 4; ++k)
        r[4 * i + k] = ((t[4 * i] * q[k] + t[4 * i + 1] * q[4 + k]) + t[4 * i + 2] * q[8 + k]) + t[4 * i + 3] * q[12 + k];
  }
  memcpy(out, r, sizeof r);
  return D2PC_OK;
}

int d2pc_rig_create(d2pc_ctx *ctx, const d2pc_rig_config *cfg, const double *q, d2pc_rig **out) {
  if (!ctx || !out) return D2PC_ERR_INVALID_ARG;
  *out = nullptr;
  if (!q) return fail(ctx, D2PC_ERR_INVALID_ARG, "q is null");
  uint64_t roi = 0;
  const int st = check(cfg, ctx->cfg.border, &roi);
  if (st != D2PC_OK) return fail(ctx, st, "bad d2pc_rig_config (d2pc_rig_geometry refuses it alike)");
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  d2pc_rig *rig = new (std::nothrow) d2pc_rig();
  QScratch scratch;
  if (!rig || !scratch.c) {
    delete rig;
    return fail(ctx, D2PC_ERR_OUT_OF_MEMORY, "out of host memory");
  }
  rig->ctx = ctx;
  rig->cfg = *cfg;
  const size_t n = size_t(cfg->n_cameras);
  rig->q.assign(q, q + 16 * n);
  std::vector<RigCal> table(n);
  for (size_t f = 0; f < n; ++f) fill_entry(scratch.c, q + 16 * f, &table[f]);
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&rig->d_table), n * sizeof(RigCal));
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&rig->d_tiles), tile_bytes(*cfg));
  if (e == hipSuccess) e = hipMemcpy(rig->d_table, table.data(), n * sizeof(RigCal), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)d2pc_rig_destroy(rig);
    return fail(ctx, e == hipErrorOutOfMemory ? D2PC_ERR_OUT_OF_MEMORY : D2PC_ERR_DEVICE, "rig allocation failed: %s",
                hipGetErrorString(e));
  }
  *out = rig;
  return D2PC_OK;
}

int d2pc_rig_destroy(d2pc_rig *rig) {
  if (!rig) return D2PC_ERR_INVALID_ARG;
  DeviceGuard guard(rig->ctx->device);
  if (rig->d_table) (void)hipFree(rig->d_table);  // (hipFree waits for the device's work)
  if (rig->d_tiles) (void)hipFree(rig->d_tiles);
  delete rig;
  return D2PC_OK;
}

int d2pc_rig_set_q(d2pc_rig *rig, int camera, const double q[16]) {
  if (!rig) return D2PC_ERR_INVALID_ARG;
  d2pc_ctx *ctx = rig->ctx;
  if (!q) return fail(ctx, D2PC_ERR_INVALID_ARG, "q is null");
  if (camera < 0 || camera >= rig->cfg.n_cameras)
    return fail(ctx, D2PC_ERR_INVALID_ARG, "camera %d is not one of the rig's %d", camera, rig->cfg.n_cameras);
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  QScratch scratch;
  if (!scratch.c) return fail(ctx, D2PC_ERR_OUT_OF_MEMORY, "out of host memory");
  RigCal e;
  fill_entry(scratch.c, q, &e);
  D2PC_HIP(ctx, hipMemcpy(rig->d_table + camera, &e, sizeof e, hipMemcpyHostToDevice));
  memcpy(rig->q.data() + 16 * size_t(camera), q, 16 * sizeof(double));  // bit copy
  return D2PC_OK;
}

int d2pc_rig_get_q(const d2pc_rig *rig, int camera, double q_out[16]) {
  if (!rig || !q_out || camera < 0 || camera >= rig->cfg.n_cameras) return D2PC_ERR_INVALID_ARG;
  memcpy(q_out, rig->q.data() + 16 * size_t(camera), 16 * sizeof(double));
  return D2PC_OK;
}

int d2pc_rig_process_device(d2pc_rig *rig, const void *d_frames, float scale, size_t row_stride, size_t frame_stride,
                            void *d_out, uint32_t *d_idx, size_t capacity, uint32_t *d_counts, uint32_t *d_offsets,
                            void *stream) {
  if (!rig) return D2PC_ERR_INVALID_ARG;
  d2pc_ctx *ctx = rig->ctx;
  const d2pc_rig_config &c = rig->cfg;
  const int n = c.n_cameras;
  if (!d_frames || !d_out) return fail(ctx, D2PC_ERR_INVALID_ARG, "null device pointer");
  if (reinterpret_cast<uintptr_t>(d_out) % 16 != 0) return fail(ctx, D2PC_ERR_INVALID_ARG, "d_out_points must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_frames) % elem_size(c.dtype) != 0)
    return fail(ctx, D2PC_ERR_INVALID_ARG, "d_frames is not aligned to its sample type");
  if (ctx->reproject_form == D2PC_FORM_CV24)
    return fail(ctx, D2PC_ERR_INVALID_ARG, "a rig has no D2PC_FORM_CV24: its per-row segments are host work per Q and per width");
  const bool compact = ctx->cfg.mode == D2PC_MODE_COMPACT;
  if (compact && (!d_counts || !d_offsets)) return fail(ctx, D2PC_ERR_INVALID_ARG, "COMPACT mode needs d_counts and d_offsets");
  uint64_t roi = 0;
  int st = check(&c, ctx->cfg.border, &roi);
  if (st != D2PC_OK) return fail(ctx, st, "%d cameras of %dx%d with border %d: beyond 2^32 points", n, c.width, c.height, ctx->cfg.border);
  if (d_idx && !index_available(c))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "no index for %d cameras of %dx%d: the batch has more than 2^32 pixels", n, c.width, c.height);
  const size_t total = size_t(roi) * size_t(n);
  if (capacity < total) return fail(ctx, D2PC_ERR_CAPACITY, "capacity of %zu points < %zu", capacity, total);
  RigArgs a;
  st = make_geom(ctx, c.dtype, scale, c.width, c.height, row_stride, frame_stride, n, size_t(roi),
                 compact ? kRigCompactPxt : kRigParityPxt, &a.geom);
  if (st != D2PC_OK) return st;
  const Plane in{d_frames, row_stride, frame_stride, size_t(c.width) * elem_size(c.dtype), c.height};
  if (!in.fits(n, Bound32::Plane)) return fail(ctx, D2PC_ERR_BAD_SIZE, "row stride / frame stride too small for %dx%d", c.width, c.height);
  const Plane pts{d_out, total * 16, 0, total * 16, 1}, idx{d_idx, total * 4, 0, total * 4, 1};
  const Plane cnt{d_counts, size_t(n) * 4, 0, size_t(n) * 4, 1}, off{d_offsets, size_t(n + 1) * 4, 0, size_t(n + 1) * 4, 1};
  // (the outputs have one "frame": their extent is a single row; the frames' hull spans all n cameras)
  auto hits = [&](const Plane &o) { return o.p && !o.empty() && overlaps(Plane{in.p, in.extent(n), 0, in.extent(n), 1}, o, 1); };
  if (hits(pts) || hits(idx) || hits(cnt) || hits(off)) return fail(ctx, D2PC_ERR_INVALID_ARG, "the frames overlap an output");
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = HIP's default stream
  if (roi == 0) {  // a border wider than the frame: no points, no launch
    if (d_counts) D2PC_HIP(ctx, hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * size_t(n), s));
    if (d_offsets) D2PC_HIP(ctx, hipMemsetAsync(d_offsets, 0, sizeof(uint32_t) * size_t(n + 1), s));
    return D2PC_OK;
  }
  a.geom.in_frame_stride = in.kernel_frame_stride(n);
  a.frames = d_frames, a.out_points = d_out, a.out_index = d_idx, a.counts = d_counts, a.offsets = d_offsets;
  a.table = rig->d_table, a.tiles = rig->d_tiles;
  a.dtype = c.dtype, a.cv4 = ctx->reproject_form == D2PC_FORM_CV4 ? 1u : 0u;
  a.frame_pixels = uint32_t(uint64_t(c.width) * uint64_t(c.height));
  a.stream = s;
  D2PC_HIP(ctx, compact ? launch_rig_compact(a) : launch_rig_parity(a));
  return D2PC_OK;
}

// ---- textured clouds (d2pc_texture_*): lives here to share this translation unit and the rig's code object ----------
void d2pc_texture_desc_init(d2pc_texture_desc *desc) {
  if (!desc) return;
  memset(desc, 0, sizeof *desc);
  desc->struct_size = sizeof *desc;
  desc->point_format = D2PC_POINT_XYZI;
  desc->texture_format = D2PC_TEX_U8;
  desc->n_frames = 1;
}

int d2pc_textured_cloud_meta_fill(int point_format, size_t n, int is_dense, d2pc_textured_cloud_meta *m) {
  if (!m) return D2PC_ERR_INVALID_ARG;
  if (point_format != D2PC_POINT_XYZI && point_format != D2PC_POINT_XYZRGB) return D2PC_ERR_BAD_DTYPE;
  if (n > 0xffffffffull / 32) return D2PC_ERR_BAD_SIZE;
  memset(m, 0, sizeof *m);
  m->height = 1;
  m->width = uint32_t(n);
  m->point_step = 32;
  m->row_step = uint32_t(32 * n);
  m->is_dense = is_dense ? 1 : 0;
  m->n_fields = 4;
  const char *names[4] = {"x", "y", "z", point_format == D2PC_POINT_XYZI ? "intensity" : "rgb"};
  for (int i = 0; i < 4; ++i) {
    strncpy(m->fields[i].name, names[i], sizeof m->fields[i].name - 1);
    m->fields[i].offset = i < 3 ? uint32_t(4 * i) : 16u;
    m->fields[i].datatype = 7;  // sensor_msgs::PointField::FLOAT32
    m->fields[i].count = 1;
  }
  return D2PC_OK;
}

int d2pc_texture_device(d2pc_ctx *ctx, const d2pc_texture_desc *d, void *stream) {
  if (!ctx) return D2PC_ERR_INVALID_ARG;
  if (!d || d->struct_size != sizeof(d2pc_texture_desc)) return fail(ctx, D2PC_ERR_INVALID_ARG, "bad d2pc_texture_desc");
  if (!d->texture || !d->points || !d->out) return fail(ctx, D2PC_ERR_INVALID_ARG, "null device pointer");
  TexArgs a;
  size_t bpp = 1;
  switch (d->texture_format) {
    case D2PC_TEX_U8: a.kind = TEX_U8; break;
    case D2PC_TEX_U16: a.kind = TEX_U16, bpp = 2; break;
    case D2PC_TEX_F32: a.kind = TEX_F32, bpp = 4; break;
    case D2PC_TEX_RGB8: a.kind = TEX_RGB8, bpp = 3; break;
    case D2PC_TEX_BGR8: a.kind = TEX_BGR8, bpp = 3; break;
    case D2PC_TEX_MONO8: a.kind = TEX_MONO8; break;
    default: return fail(ctx, D2PC_ERR_BAD_DTYPE, "unknown texture format %d", d->texture_format);
  }
  const bool rgb = a.kind >= TEX_RGB8;
  if (d->point_format != (rgb ? D2PC_POINT_XYZRGB : D2PC_POINT_XYZI))
    return fail(ctx, D2PC_ERR_BAD_DTYPE, "texture format %d does not belong to point format %d", d->texture_format, d->point_format);
  if (d->width <= 0 || d->height <= 0 || d->n_frames <= 0 || d->n_frames > 65535 || d->border < 0)
    return fail(ctx, D2PC_ERR_BAD_SIZE, "%d frames of %dx%d, border %d", d->n_frames, d->width, d->height, d->border);
  const uint64_t frame_pixels = uint64_t(d->width) * uint64_t(d->height);
  const bool merged = d->merged != 0;
  if (frame_pixels > (uint64_t(1) << 31) || (merged && frame_pixels * uint64_t(d->n_frames) > (uint64_t(1) << 32)))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "%d frames of %dx%d: a pixel index does not fit 32 bits", d->n_frames, d->width, d->height);
  if (d->cloud_points == 0 || uint64_t(d->cloud_points) >= (uint64_t(1) << 32))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "cloud_points of %zu: a point's position is 32 bits", d->cloud_points);
  if (!d->index) {
    if (merged) return fail(ctx, D2PC_ERR_INVALID_ARG, "a merged cloud needs its index");
    if (d->cloud_points != d2pc_roi_points(d->width, d->height, d->border))
      return fail(ctx, D2PC_ERR_BAD_SIZE, "no index: cloud_points must be the %zu ROI points", d2pc_roi_points(d->width, d->height, d->border));
  }
  const int n_clouds = merged ? 1 : d->n_frames;
  const size_t cp = d->cloud_points;
  if (n_clouds > 1 && (d->points_frame_stride_points < cp || d->out_frame_stride_points < cp))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "a frame stride is smaller than cloud_points (%zu)", cp);
  // 65,535 clouds x 2^40 records x 32 B and 65,535 planes x 2^46 B stay below 2^62: no hull below can wrap
  constexpr size_t kMaxStride = size_t(1) << 40, kMaxTexStride = size_t(1) << 46;
  if (n_clouds > 1 && (d->points_frame_stride_points > kMaxStride || d->out_frame_stride_points > kMaxStride))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "a frame stride beyond 2^40 points");
  if (d->n_frames > 1 && d->tex_frame_stride > kMaxTexStride) return fail(ctx, D2PC_ERR_BAD_SIZE, "tex_frame_stride beyond 2^46 bytes");
  auto misaligned = [](const void *p, size_t to) { return reinterpret_cast<uintptr_t>(p) % to != 0; };
  if (misaligned(d->points, 16) || misaligned(d->out, 16)) return fail(ctx, D2PC_ERR_INVALID_ARG, "points and out must be 16-byte aligned");
  if (misaligned(d->index, 4) || misaligned(d->counts, 4)) return fail(ctx, D2PC_ERR_INVALID_ARG, "index / counts are not aligned to 4 bytes");
  const size_t sample = bpp == 3 ? 1 : bpp;
  if (misaligned(d->texture, sample) || d->tex_pitch % sample != 0 || (d->n_frames > 1 && d->tex_frame_stride % sample != 0))
    return fail(ctx, D2PC_ERR_INVALID_ARG, "the texture is not aligned to its sample type");
  const Plane tex{d->texture, d->tex_pitch, d->tex_frame_stride, size_t(d->width) * bpp, d->height};
  if (!tex.fits(d->n_frames, Bound32::Pitch))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "texture pitch / frame stride too small for %dx%d (or a pitch beyond 2^32)", d->width, d->height);
  // the clouds as planes of one row, so that extent() is their hull over n_clouds
  const Plane pts{d->points, cp * 16, d->points_frame_stride_points * 16, cp * 16, 1};
  const Plane idx{d->index, cp * 4, d->points_frame_stride_points * 4, cp * 4, 1};
  const Plane cnt{d->counts, size_t(n_clouds) * 4, 0, size_t(n_clouds) * 4, 1};
  const Plane out{d->out, cp * 32, d->out_frame_stride_points * 32, cp * 32, 1};
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(out.p), o1 = o0 + out.extent(n_clouds);
  auto hits = [&](const Plane &in, int n) {
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(in.p);
    return in.p && i0 < o1 && o0 < i0 + in.extent(n);
  };
  if (hits(tex, d->n_frames) || hits(pts, n_clouds) || hits(idx, n_clouds) || hits(cnt, 1))
    return fail(ctx, D2PC_ERR_INVALID_ARG, "out overlaps an input");
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  a.tex = static_cast<const uint8_t *>(d->texture), a.points = d->points, a.index = d->index, a.counts = d->counts, a.out = d->out;
  a.tex_pitch = uint32_t(d->tex_pitch), a.tex_frame_stride = tex.kernel_frame_stride(d->n_frames);
  a.points_stride = n_clouds > 1 ? d->points_frame_stride_points : 0, a.out_stride = n_clouds > 1 ? d->out_frame_stride_points : 0;
  a.pixel_limit = merged ? frame_pixels * uint64_t(d->n_frames) : frame_pixels;
  a.cloud_points = uint32_t(cp), a.n_clouds = uint32_t(n_clouds), a.merged = merged ? 1u : 0u;
  a.width = uint32_t(d->width), a.frame_pixels = uint32_t(frame_pixels), a.border = uint32_t(d->border);
  a.roi_w = d->index ? 1u : uint32_t(d->width - 2 * d->border);  // (no index: the ROI is not empty, checked above)
  a.div_w = make_fastdiv(a.width), a.div_frame = make_fastdiv(a.frame_pixels), a.div_roi_w = make_fastdiv(a.roi_w);
  a.stream = static_cast<hipStream_t>(stream);  // NULL = HIP's default stream
  D2PC_HIP(ctx, launch_texture(a));
  return D2PC_OK;
}

}  // extern "C"
