// d2pc_capi_node.hip -- the depth_map_fusion node (reference src/depth_map_fusion.cpp) as a session of the C ABI:
// d2pc_fusion_node_* of include/d2pc.h.  Host code only; the kernels are those of d2pc_colorize / d2pc_score /
// d2pc_fusion .hip, reached through the ABI's own device entry points (so every launch is validated as a caller's
// would be), and the single-launch DisparityCb2 of d2pc_node.hip.
#include "d2pc_ctx.hpp"

using namespace d2pc;
using namespace d2pc::host;

namespace {
constexpr uint32_t kNodeMagic = 0x64327066u;  // "d2pf"
}

struct d2pc_fusion_node {
  uint32_t magic = kNodeMagic;
  d2pc_ctx *ctx = nullptr;
  d2pc_fusion_node_config cfg{};
  d2pc_fusion_node_geometry_t geo{};
  // device planes; tight rows (pitch = width x channels), the pairs of a batch one plane apart
  uint8_t *rot = nullptr;                 // camera 2's score frame, rotated: cols rows of `rows` pixels
  uint8_t *depth[2] = {nullptr, nullptr};
  uint8_t *score1 = nullptr, *spare = nullptr, *score2 = nullptr;  // score1 <-> spare swap on every fusion (:113)
  uint8_t *color[2] = {nullptr, nullptr};
  uint8_t *fused = nullptr, *gradient = nullptr;
  uint8_t *stage = nullptr;               // the host entry's upload of the incoming frame
  uint32_t *table = nullptr;              // colour table of the single-launch kernel
  bool have[4] = {false, false, false, false};  // depth_1, depth_2, score_1, score_2 (:106-109)
};

namespace {

bool cfg_ok(const d2pc_fusion_node_config *c) { return c && c->struct_size == sizeof(d2pc_fusion_node_config); }

// 64-bit: |INT_MIN| has no int
bool offsets_refused(const d2pc_fusion_node_config &c) {
  const int64_t ax = c.offset_x < 0 ? -int64_t(c.offset_x) : int64_t(c.offset_x);
  const int64_t ay = c.offset_y < 0 ? -int64_t(c.offset_y) : int64_t(c.offset_y);
  return ax > ay;
}

int geometry(const d2pc_fusion_node_config &c, d2pc_fusion_node_geometry_t *g) {
  memset(g, 0, sizeof *g);
  if (c.rule < 0 || c.rule >= FUSE_RULE_COUNT) return D2PC_ERR_INVALID_ARG;
  if (c.score_form != D2PC_SCORE_FORM_CV4 && c.score_form != D2PC_SCORE_FORM_CV3) return D2PC_ERR_INVALID_ARG;
  if (c.cols <= 0 || c.rows <= 0 || c.batch < 1 || c.batch > 65535) return D2PC_ERR_BAD_SIZE;
  if (c.crop_left < 0 || c.crop_right < 0 || c.crop_top < 0 || c.crop_bottom < 0) return D2PC_ERR_BAD_SIZE;
  int n1 = 0, n2 = 0;
  // publishFusedDepthMap re-crops the incoming frame with cropToSquare(image) (:106): its arguments are 0 but the side
  // still uses the member offset_y_ (:253), so that square has min(cols, rows) - |offset_y| pixels a side while the
  // loop of :115-123 fuses only min(cols, rows) - max(|offset_x|, |offset_y|) of them.  With |offset_x| > |offset_y|
  // the reference therefore publishes a larger fused map whose last rows and columns are raw, unrotated camera-2
  // pixels run through the median (200 x 140 with 9 / -6: 94 x 94 where the fused square gives 91 x 91).  Not
  // reproduced: refused.
  if (offsets_refused(c)) return D2PC_ERR_BAD_SIZE;
  // camera 1: cropToSquare(image, offset_x, offset_y); camera 2: of the ROTATED image (rows x cols) with the negated
  // offsets -- while the side length still uses the member offset_y_ (:253)
  if (d2pc_crop_to_square(c.cols, c.rows, c.offset_x, c.offset_y, c.offset_y, &g->x1, &g->y1, &n1) != D2PC_OK ||
      d2pc_crop_to_square(c.rows, c.cols, -c.offset_x, -c.offset_y, c.offset_y, &g->x2, &g->y2, &n2) != D2PC_OK)
    return D2PC_ERR_BAD_SIZE;
  if (n1 != n2 || n1 < 11) return D2PC_ERR_BAD_SIZE;
  g->n = n1;
  g->fused_width = n1 - c.crop_left - c.crop_right;
  g->fused_height = n1 - c.crop_top - c.crop_bottom;
  if (g->fused_width < 1 || g->fused_height < 1) return D2PC_ERR_BAD_SIZE;
  const size_t sq = size_t(n1) * size_t(n1) * size_t(c.batch);
  const size_t fu = size_t(g->fused_width) * size_t(g->fused_height) * size_t(c.batch);
  g->topic_bytes[D2PC_TOPIC_CROPPED_DEPTH_1] = g->topic_bytes[D2PC_TOPIC_CROPPED_DEPTH_2] = 3 * sq;
  g->topic_bytes[D2PC_TOPIC_CROPPED_SCORE_1] = g->topic_bytes[D2PC_TOPIC_CROPPED_SCORE_2] = sq;
  g->topic_bytes[D2PC_TOPIC_COMBINED_SCORE] = sq;
  g->topic_bytes[D2PC_TOPIC_FUSED_DEPTH_MAP] = fu;
  g->topic_bytes[D2PC_TOPIC_GRADIENT] = 3 * fu;
  return D2PC_OK;
}

bool node_ok(const d2pc_fusion_node *n) { return n && n->magic == kNodeMagic && n->ctx; }

void free_planes(d2pc_fusion_node *n) {
  void *all[] = {n->rot, n->depth[0], n->depth[1], n->score1, n->spare, n->score2, n->color[0], n->color[1],
                 n->fused, n->gradient, n->stage, n->table};
  for (void *p : all)
    if (p) (void)hipFree(p);
}

// which topics the callback `which` publishes in the node's present state
uint32_t publishes(const d2pc_fusion_node *n, int which) {
  switch (which) {
    case D2PC_NODE_DISPARITY_1: return 1u << D2PC_TOPIC_CROPPED_DEPTH_1;
    case D2PC_NODE_MATCHING_SCORE_1: return 1u << D2PC_TOPIC_CROPPED_SCORE_1;
    case D2PC_NODE_MATCHING_SCORE_2: return 1u << D2PC_TOPIC_CROPPED_SCORE_2;
    default:
      return (1u << D2PC_TOPIC_CROPPED_DEPTH_2) |
             ((n->have[0] && n->have[2] && n->have[3])
                  ? (1u << D2PC_TOPIC_COMBINED_SCORE) | (1u << D2PC_TOPIC_GRADIENT) | (1u << D2PC_TOPIC_FUSED_DEPTH_MAP)
                  : 0u);
  }
}

// one of the node's own planes: w x h pixels of `ch` bytes, rows and frames packed
Plane tight(const void *p, int w, int h, int ch = 1) {
  const size_t row = size_t(w) * size_t(ch);
  return Plane{p, row, row * size_t(h), row, h};
}

void describe(const d2pc_fusion_node *n, int id, d2pc_fusion_node_topic *t) {
  const int sq = n->geo.n, fw = n->geo.fused_width, fh = n->geo.fused_height;
  void *data = nullptr;
  int w = sq, h = sq, ch = 1;
  switch (id) {
    case D2PC_TOPIC_CROPPED_DEPTH_1: data = n->color[0], ch = 3; break;
    case D2PC_TOPIC_CROPPED_DEPTH_2: data = n->color[1], ch = 3; break;
    case D2PC_TOPIC_CROPPED_SCORE_1: data = n->score1; break;
    case D2PC_TOPIC_CROPPED_SCORE_2: data = n->score2; break;
    case D2PC_TOPIC_COMBINED_SCORE: data = n->score1; break;  // after the swap: the combined plane IS camera 1's score
    case D2PC_TOPIC_FUSED_DEPTH_MAP: data = n->fused, w = fw, h = fh; break;
    default: data = n->gradient, w = fw, h = fh, ch = 3; break;
  }
  const Plane pl = tight(data, w, h, ch);
  t->data = data, t->pitch = pl.pitch, t->frame_stride = pl.frame_stride;
  t->width = w, t->height = h, t->channels = ch, t->reserved = 0;
}

// the view (x, y, w, h) of `src` (8-bit frames of src.row_bytes x src.rows pixels), rotated first or not, into tight planes
int colorize(d2pc_fusion_node *n, const Plane &src, int rotate, int x, int y, int w, int h, uint8_t *gray, uint8_t *rgb,
             void *stream) {
  d2pc_colorize_desc d;
  d2pc_colorize_desc_init(&d);
  d.rotate_cw = rotate, d.cols = int(src.row_bytes), d.rows = src.rows, d.n_frames = n->cfg.batch;
  d.x = x, d.y = y, d.w = w, d.h = h;
  const Plane g = tight(gray, w, h), c = tight(rgb, w, h, 3);
  d.src = src.p, d.src_pitch = src.pitch, d.src_frame_stride = src.frame_stride;
  d.gray = gray, d.gray_pitch = g.pitch, d.gray_frame_stride = g.frame_stride;
  d.rgb = rgb, d.rgb_pitch = c.pitch, d.rgb_frame_stride = c.frame_stride;
  return d2pc_colorize_device(n->ctx, &d, stream);
}

int score_filter(d2pc_fusion_node *n, const Plane &src, int x, int y, int direction, uint8_t *out, void *stream) {
  d2pc_score_filter_desc d;
  d2pc_score_filter_desc_init(&d);
  d.direction = direction, d.form = n->cfg.score_form, d.width = int(src.row_bytes), d.height = src.rows, d.n_frames = n->cfg.batch;
  d.x = x, d.y = y, d.n = n->geo.n;
  const Plane o = tight(out, d.n, d.n);
  d.src = src.p, d.src_pitch = src.pitch, d.src_frame_stride = src.frame_stride;
  d.out = out, d.out_pitch = o.pitch, d.out_frame_stride = o.frame_stride;
  return d2pc_score_filter_device(n->ctx, &d, stream);
}

// publishFusedDepthMap (:102-135) behind camera 2's view: either inside the single launch or as two more launches
int disparity_2(d2pc_fusion_node *n, const Plane &frame, bool fuse, void *stream) {
  const d2pc_fusion_node_config &c = n->cfg;
  const d2pc_fusion_node_geometry_t &g = n->geo;
  const Plane sq = tight(nullptr, g.n, g.n), sq3 = tight(nullptr, g.n, g.n, 3);
  const Plane fu = tight(n->fused, g.fused_width, g.fused_height), fu3 = tight(nullptr, g.fused_width, g.fused_height, 3);
  if (fuse && c.single_launch && c.rule == D2PC_FUSE_GRAD_FILTER) {
    DeviceGuard guard(n->ctx->device);
    if (!guard.ok) return fail(n->ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", n->ctx->device);
    NodeFuseArgs a;
    a.frame2 = static_cast<const uint8_t *>(frame.p), a.frame2_pitch = frame.pitch, a.frame2_frame_stride = frame.frame_stride;
    a.depth1 = n->depth[0], a.score1 = n->score1, a.score2 = n->score2, a.spare = n->spare;
    a.depth1_pitch = a.score1_pitch = a.score2_pitch = a.spare_pitch = sq.pitch;
    a.depth1_frame_stride = a.score1_frame_stride = a.score2_frame_stride = a.spare_frame_stride = sq.frame_stride;
    a.rgb2 = n->color[1], a.rgb2_pitch = sq3.pitch, a.rgb2_frame_stride = sq3.frame_stride;
    a.fused = n->fused, a.fused_pitch = fu.pitch, a.fused_frame_stride = fu.frame_stride;
    a.gradient = n->gradient, a.gradient_pitch = fu3.pitch, a.gradient_frame_stride = fu3.frame_stride;
    a.table = n->table;
    a.rows = c.rows, a.x2 = g.x2, a.y2 = g.y2, a.n = g.n;
    a.crop_left = c.crop_left, a.crop_top = c.crop_top, a.out_width = g.fused_width, a.out_height = g.fused_height;
    a.n_frames = c.batch;
    D2PC_HIP(n->ctx, launch_node_fuse(a, static_cast<hipStream_t>(stream)));
    return D2PC_OK;
  }
  int st = colorize(n, frame, 1, g.x2, g.y2, g.n, g.n, n->depth[1], n->color[1], stream);
  if (st != D2PC_OK || !fuse) return st;
  d2pc_fuse_desc d;
  d2pc_fuse_desc_init(&d);
  d.rule = c.rule, d.width = d.height = g.n, d.n_frames = c.batch;
  d.crop_left = c.crop_left, d.crop_right = c.crop_right, d.crop_top = c.crop_top, d.crop_bottom = c.crop_bottom;
  const uint8_t *in[6] = {n->depth[0], n->depth[1], n->score1, n->score2, n->score1, n->score2};  // score and grad: one plane (:77,:96)
  for (int p = 0; p < 6; ++p) d.planes[p] = in[p], d.pitch[p] = sq.pitch, d.frame_stride[p] = sq.frame_stride;
  d.fused = n->fused, d.fused_pitch = fu.pitch, d.fused_frame_stride = fu.frame_stride;
  d.combined = n->spare, d.combined_pitch = sq.pitch, d.combined_frame_stride = sq.frame_stride;
  if ((st = d2pc_fuse_device(n->ctx, &d, stream)) != D2PC_OK) return st;
  return colorize(n, fu, 0, 0, 0, g.fused_width, g.fused_height, nullptr, n->gradient, stream);
}

}  // namespace

extern "C" {

void d2pc_fusion_node_config_init(d2pc_fusion_node_config *cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = sizeof *cfg;
  cfg->rule = D2PC_FUSE_GRAD_FILTER;       // src/depth_map_fusion.cpp:159
  cfg->score_form = D2PC_SCORE_FORM_CV4;
  cfg->batch = 1;
  cfg->crop_left = 0, cfg->crop_right = 40, cfg->crop_top = 30, cfg->crop_bottom = 10;  // :130
  cfg->single_launch = 1;
}

int d2pc_fusion_node_geometry(const d2pc_fusion_node_config *cfg, d2pc_fusion_node_geometry_t *out) {
  if (!cfg_ok(cfg) || !out) return D2PC_ERR_INVALID_ARG;
  return geometry(*cfg, out);
}

int d2pc_fusion_node_create(d2pc_ctx *ctx, const d2pc_fusion_node_config *cfg, d2pc_fusion_node **out) {
  if (!ctx || !out) return D2PC_ERR_INVALID_ARG;
  *out = nullptr;
  if (!cfg_ok(cfg)) return fail(ctx, D2PC_ERR_INVALID_ARG, "bad d2pc_fusion_node_config");
  d2pc_fusion_node_geometry_t g;
  const int st = geometry(*cfg, &g);
  if (st == D2PC_ERR_BAD_SIZE && offsets_refused(*cfg))
    return fail(ctx, st, "fusion node %dx%d: |offset_x| (%d) exceeds |offset_y| (%d): the reference fuses a smaller square than it "
                "publishes there; not supported", cfg->cols, cfg->rows, cfg->offset_x, cfg->offset_y);
  if (st != D2PC_OK)
    return fail(ctx, st, "fusion node %dx%d offsets %d/%d: bad configuration or a square too small for the filter and the crop",
                cfg->cols, cfg->rows, cfg->offset_x, cfg->offset_y);
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  d2pc_fusion_node *n = new (std::nothrow) d2pc_fusion_node;
  if (!n) return fail(ctx, D2PC_ERR_OUT_OF_MEMORY, "out of host memory");
  n->ctx = ctx, n->cfg = *cfg, n->geo = g;
  const size_t B = size_t(cfg->batch), frame = size_t(cfg->cols) * size_t(cfg->rows) * B;
  const size_t sq = g.topic_bytes[D2PC_TOPIC_CROPPED_SCORE_1], fu = g.topic_bytes[D2PC_TOPIC_FUSED_DEPTH_MAP];
  struct { uint8_t **p; size_t bytes; } want[] = {
      {&n->rot, frame}, {&n->depth[0], sq}, {&n->depth[1], sq}, {&n->score1, sq}, {&n->spare, sq}, {&n->score2, sq},
      {&n->color[0], 3 * sq}, {&n->color[1], 3 * sq}, {&n->fused, fu}, {&n->gradient, 3 * fu}, {&n->stage, frame}};
  hipError_t e = hipSuccess;
  for (auto &w : want)
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(w.p), w.bytes);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&n->table), 256 * sizeof(uint32_t));
  if (e == hipSuccess) {
    uint8_t t[768];
    uint32_t packed[256];
    colorize_table(t);
    for (int i = 0; i < 256; ++i) packed[i] = uint32_t(t[3 * i]) | (uint32_t(t[3 * i + 1]) << 8) | (uint32_t(t[3 * i + 2]) << 16);
    e = hipMemcpy(n->table, packed, sizeof packed, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    free_planes(n);
    n->magic = 0;
    delete n;
    return fail(ctx, e == hipErrorOutOfMemory ? D2PC_ERR_OUT_OF_MEMORY : D2PC_ERR_DEVICE, "fusion node buffers: %s",
                hipGetErrorString(e));
  }
  *out = n;
  return D2PC_OK;
}

int d2pc_fusion_node_destroy(d2pc_fusion_node *node) {
  if (!node_ok(node)) return D2PC_ERR_INVALID_ARG;
  DeviceGuard guard(node->ctx->device);
  (void)hipDeviceSynchronize();  // launches of any stream may still use the planes
  free_planes(node);
  node->magic = 0;
  delete node;
  return D2PC_OK;
}

int d2pc_fusion_node_callback_device(d2pc_fusion_node *node, int which, const void *d_frame, size_t pitch,
                                     size_t frame_stride, d2pc_fusion_node_topics *out, void *stream) {
  if (!node_ok(node)) return D2PC_ERR_INVALID_ARG;
  d2pc_ctx *ctx = node->ctx;
  if (which < D2PC_NODE_DISPARITY_1 || which > D2PC_NODE_MATCHING_SCORE_2)
    return fail(ctx, D2PC_ERR_INVALID_ARG, "unknown callback %d", which);
  if (!d_frame || !out || out->struct_size != sizeof(d2pc_fusion_node_topics))
    return fail(ctx, D2PC_ERR_INVALID_ARG, "null frame or bad d2pc_fusion_node_topics");
  const d2pc_fusion_node_config &c = node->cfg;
  const d2pc_fusion_node_geometry_t &g = node->geo;
  Plane frame{d_frame, pitch, frame_stride, size_t(c.cols), c.rows};
  if (!frame.fits(c.batch, Bound32::Pitch))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "frame pitch / frame stride too small for %dx%d", c.cols, c.rows);
  frame.frame_stride = frame.kernel_frame_stride(c.batch);
  const uint32_t mask = publishes(node, which);
  int st = D2PC_OK;
  switch (which) {
    case D2PC_NODE_DISPARITY_1:
      st = colorize(node, frame, 0, g.x1, g.y1, g.n, g.n, node->depth[0], node->color[0], stream);
      break;
    case D2PC_NODE_MATCHING_SCORE_1:
      st = score_filter(node, frame, g.x1, g.y1, 0, node->score1, stream);
      break;
    case D2PC_NODE_MATCHING_SCORE_2: {
      const Plane rot = tight(node->rot, c.rows, c.cols);
      st = d2pc_rotate_cw_device(ctx, d_frame, c.cols, c.rows, pitch, frame.frame_stride, c.batch, node->rot, rot.pitch,
                                 rot.frame_stride, stream);
      if (st == D2PC_OK) st = score_filter(node, rot, g.x2, g.y2, 1, node->score2, stream);
      break;
    }
    default: {
      const bool fuse = (mask >> D2PC_TOPIC_FUSED_DEPTH_MAP) & 1u;
      st = disparity_2(node, frame, fuse, stream);
      // cropped_score_combined_ IS cropped_score_1_ (:113): from now on camera 1's score / grad plane is the combined one
      if (st == D2PC_OK && fuse) std::swap(node->score1, node->spare);
      break;
    }
  }
  if (st != D2PC_OK) return st;
  node->have[which == D2PC_NODE_DISPARITY_1 ? 0 : which == D2PC_NODE_DISPARITY_2 ? 1 : which == D2PC_NODE_MATCHING_SCORE_1 ? 2 : 3] = true;
  memset(out->topic, 0, sizeof out->topic);
  out->published = mask;
  for (int id = 0; id < D2PC_NODE_TOPICS; ++id)
    if ((mask >> id) & 1u) describe(node, id, &out->topic[id]);
  return D2PC_OK;
}

int d2pc_fusion_node_callback(d2pc_fusion_node *node, int which, const void *host_frame, size_t pitch,
                              d2pc_fusion_node_host_topics *io) {
  if (!node_ok(node)) return D2PC_ERR_INVALID_ARG;
  d2pc_ctx *ctx = node->ctx;
  if (which < D2PC_NODE_DISPARITY_1 || which > D2PC_NODE_MATCHING_SCORE_2)
    return fail(ctx, D2PC_ERR_INVALID_ARG, "unknown callback %d", which);
  if (!host_frame || !io || io->struct_size != sizeof(d2pc_fusion_node_host_topics))
    return fail(ctx, D2PC_ERR_INVALID_ARG, "null frame or bad d2pc_fusion_node_host_topics");
  const d2pc_fusion_node_config &c = node->cfg;
  if (pitch < size_t(c.cols)) return fail(ctx, D2PC_ERR_BAD_SIZE, "frame pitch smaller than %d columns", c.cols);
  const uint32_t mask = publishes(node, which);
  for (int id = 0; id < D2PC_NODE_TOPICS; ++id)  // before anything is enqueued: a refused call leaves the node as it was
    if (((mask >> id) & 1u) && io->data[id] && io->capacity[id] < node->geo.topic_bytes[id])
      return fail(ctx, D2PC_ERR_CAPACITY, "buffer of topic %d holds %zu bytes, %zu needed", id, io->capacity[id],
                  node->geo.topic_bytes[id]);
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  hipStream_t s = ctx->stream;
  SyncOnExit sync(s);
  const size_t cols = size_t(c.cols), rows = size_t(c.rows) * size_t(c.batch);
  D2PC_HIP(ctx, hipMemcpy2DAsync(node->stage, cols, host_frame, pitch, cols, rows, hipMemcpyHostToDevice, s));
  d2pc_fusion_node_topics dev;
  dev.struct_size = sizeof dev;
  const int st = d2pc_fusion_node_callback_device(node, which, node->stage, cols, cols * size_t(c.rows), &dev, s);
  if (st != D2PC_OK) return st;
  io->published = dev.published;
  for (int id = 0; id < D2PC_NODE_TOPICS; ++id) {
    const d2pc_fusion_node_topic &t = dev.topic[id];
    const bool pub = (dev.published >> id) & 1u;
    io->bytes[id] = pub ? node->geo.topic_bytes[id] : 0;
    io->width[id] = t.width, io->height[id] = t.height, io->channels[id] = t.channels;
    if (pub && io->data[id]) D2PC_HIP(ctx, hipMemcpyAsync(io->data[id], t.data, io->bytes[id], hipMemcpyDeviceToHost, s));
  }
  sync.armed = false;
  D2PC_HIP(ctx, hipStreamSynchronize(s));
  return D2PC_OK;
}

}  // extern "C"
