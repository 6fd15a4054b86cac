// d2pc_capi_fusion.hip -- SURVEY.md section 8(f) #4: the per-pixel loop of publishFusedDepthMap
// (reference src/depth_map_fusion.cpp:113-130), rotateMat, cropToSquare's arithmetic, the matching-score
// pre-filter of MatchingScoreCb1/2 (:64-99) and colorizeDepth with the view of DisparityCb1/2 (:45-61, :306-360).
#include "d2pc_ctx.hpp"

using namespace d2pc;
using namespace d2pc::host;

extern "C" {

// ---------------------------------------------------------------------------
// Depth-map fusion inner loop
// ---------------------------------------------------------------------------
void d2pc_fuse_desc_init(d2pc_fuse_desc *desc) {
  if (!desc) return;
  memset(desc, 0, sizeof *desc);
  desc->struct_size = sizeof *desc;
  desc->rule = D2PC_FUSE_GRAD_FILTER;  // src/depth_map_fusion.cpp:159
  desc->n_frames = 1;
  desc->crop_left = 0;                 // src/depth_map_fusion.cpp:130
  desc->crop_right = 40;
  desc->crop_top = 30;
  desc->crop_bottom = 10;
}

int d2pc_crop_to_square(int cols, int rows, int offset_x, int offset_y, int member_offset_y, int *x, int *y, int *n) {
  if (!x || !y || !n || cols <= 0 || rows <= 0) return D2PC_ERR_INVALID_ARG;
  const int ax = offset_x < 0 ? -offset_x : offset_x, ay = offset_y < 0 ? -offset_y : offset_y;
  const int am = member_offset_y < 0 ? -member_offset_y : member_offset_y;
  const int free_cols = cols - ax, free_rows = rows - ay;
  *n = (cols < rows ? cols : rows) - (ax > am ? ax : am);
  const bool portrait = free_cols < free_rows;
  const int sx = portrait ? offset_x : offset_x + (free_cols - free_rows) / 2;
  const int sy = portrait ? offset_y + (free_rows - free_cols) / 2 : offset_y;
  *x = sx > 0 ? sx : 0;
  *y = sy > 0 ? sy : 0;
  // cv::Mat::operator()(Rect) asserts that the rectangle lies inside the image
  if (*n <= 0 || *x + *n > cols || *y + *n > rows) return D2PC_ERR_BAD_SIZE;
  return D2PC_OK;
}

int d2pc_fuse_device(d2pc_ctx *ctx, const d2pc_fuse_desc *desc, void *stream) {
  if (!ctx) return D2PC_ERR_INVALID_ARG;
  if (!desc || desc->struct_size != sizeof(d2pc_fuse_desc)) return fail(ctx, D2PC_ERR_INVALID_ARG, "bad d2pc_fuse_desc");
  const d2pc_fuse_desc &d = *desc;
  if (d.rule < 0 || d.rule >= FUSE_RULE_COUNT) return fail(ctx, D2PC_ERR_INVALID_ARG, "unknown fusion rule %d", d.rule);
  if (d.width <= 0 || d.height <= 0 || d.n_frames <= 0 || d.n_frames > 65535)
    return fail(ctx, D2PC_ERR_BAD_SIZE, "bad size %dx%d x%d", d.width, d.height, d.n_frames);
  if (d.crop_left < 0 || d.crop_right < 0 || d.crop_top < 0 || d.crop_bottom < 0 ||
      d.crop_left + d.crop_right > d.width || d.crop_top + d.crop_bottom > d.height)
    return fail(ctx, D2PC_ERR_BAD_SIZE, "crop %d/%d/%d/%d does not fit %dx%d", d.crop_left, d.crop_right, d.crop_top,
                d.crop_bottom, d.width, d.height);
  if (!d.fused) return fail(ctx, D2PC_ERR_INVALID_ARG, "null fused output");
  const int n_in = d.combined ? 6 : 4, nf = d.n_frames;
  Plane in[6];
  for (int p = 0; p < n_in; ++p) {
    in[p] = Plane{d.planes[p], d.pitch[p], d.frame_stride[p], size_t(d.width), d.height};
    if (!in[p].p) return fail(ctx, D2PC_ERR_INVALID_ARG, "input plane %d is null", p);
    if (!in[p].fits(nf, Bound32::Plane))
      return fail(ctx, D2PC_ERR_BAD_SIZE, "pitch / frame stride of plane %d too small (or plane >= 4 GiB)", p);
  }
  const int ow = d.width - d.crop_left - d.crop_right, oh = d.height - d.crop_top - d.crop_bottom;
  const Plane fused{d.fused, d.fused_pitch, d.fused_frame_stride, size_t(ow), oh};  // empty when the crop leaves nothing
  const Plane combined{d.combined, d.combined_pitch, d.combined_frame_stride, size_t(d.width), d.height};
  if (!fused.empty() && !fused.fits(nf, Bound32::Plane))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "fused pitch / frame stride too small (or plane >= 4 GiB)");
  if (combined.p && !combined.fits(nf, Bound32::Plane))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "combined pitch / frame stride too small (or plane >= 4 GiB)");
  if (overlaps(fused, combined, nf)) return fail(ctx, D2PC_ERR_INVALID_ARG, "fused and combined outputs overlap");
  for (int p = 0; p < n_in; ++p)
    if (overlaps(in[p], fused, nf) || overlaps(in[p], combined, nf))
      return fail(ctx, D2PC_ERR_INVALID_ARG, "an output overlaps input plane %d (in-place fusion is not supported)", p);
  if (fused.empty() && !combined.p) return D2PC_OK;  // nothing to write
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  FuseArgs a;
  for (int p = 0; p < 6; ++p) {
    const Plane &q = in[p < n_in ? p : 0];  // unused grad planes: any valid pointer
    a.in[p] = static_cast<const uint8_t *>(q.p);
    a.in_pitch[p] = uint32_t(q.pitch);
    a.in_frame_stride[p] = q.kernel_frame_stride(nf);
  }
  a.fused = static_cast<uint8_t *>(d.fused);
  a.fused_pitch = uint32_t(fused.pitch);
  a.fused_frame_stride = fused.kernel_frame_stride(nf);
  a.combined = static_cast<uint8_t *>(d.combined);
  a.combined_pitch = uint32_t(combined.pitch);
  a.combined_frame_stride = combined.kernel_frame_stride(nf);
  a.width = uint32_t(d.width);
  a.height = uint32_t(d.height);
  a.n_frames = uint32_t(d.n_frames);
  a.rule = d.rule;
  a.crop_left = uint32_t(d.crop_left);
  a.crop_top = uint32_t(d.crop_top);
  a.out_width = uint32_t(ow);  // (the crop checks above: neither is negative)
  a.out_height = uint32_t(oh);
  D2PC_HIP(ctx, launch_fuse(a, static_cast<hipStream_t>(stream), ctx->fuse_rows));
  return D2PC_OK;
}

int d2pc_rotate_cw_device(d2pc_ctx *ctx, const void *d_src, int cols, int rows, size_t src_pitch,
                          size_t src_frame_stride, int n_frames, void *d_dst, size_t dst_pitch,
                          size_t dst_frame_stride, void *stream) {
  if (!ctx) return D2PC_ERR_INVALID_ARG;
  if (!d_src || !d_dst) return fail(ctx, D2PC_ERR_INVALID_ARG, "null device pointer");
  if (cols <= 0 || rows <= 0 || n_frames <= 0 || n_frames > 65535)
    return fail(ctx, D2PC_ERR_BAD_SIZE, "bad size %dx%d x%d", cols, rows, n_frames);
  const Plane src{d_src, src_pitch, src_frame_stride, size_t(cols), rows};
  const Plane dst{d_dst, dst_pitch, dst_frame_stride, size_t(rows), cols};
  if (!src.fits(n_frames, Bound32::Pitch) || !dst.fits(n_frames, Bound32::Pitch))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "pitch / frame stride too small (src rows are %d, dst rows %d pixels)", cols, rows);
  if (overlaps(src, dst, n_frames)) return fail(ctx, D2PC_ERR_INVALID_ARG, "source and destination overlap");
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  RotateArgs a;
  a.src = static_cast<const uint8_t *>(d_src);
  a.dst = static_cast<uint8_t *>(d_dst);
  a.src_pitch = uint32_t(src_pitch);
  a.dst_pitch = uint32_t(dst_pitch);
  a.src_frame_stride = src.kernel_frame_stride(n_frames);
  a.dst_frame_stride = dst.kernel_frame_stride(n_frames);
  a.cols = uint32_t(cols);
  a.rows = uint32_t(rows);
  a.n_frames = uint32_t(n_frames);
  D2PC_HIP(ctx, launch_rotate_cw(a, static_cast<hipStream_t>(stream)));
  return D2PC_OK;
}

// ---------------------------------------------------------------------------
// Matching-score pre-filter (src/depth_map_fusion.cpp:64-99)
// ---------------------------------------------------------------------------
void d2pc_score_filter_desc_init(d2pc_score_filter_desc *desc) {
  if (!desc) return;
  memset(desc, 0, sizeof *desc);
  desc->struct_size = sizeof *desc;
  desc->direction = 0;
  desc->form = D2PC_SCORE_FORM_CV4;
  desc->n_frames = 1;
}

int d2pc_score_filter_device(d2pc_ctx *ctx, const d2pc_score_filter_desc *desc, void *stream) {
  if (!ctx) return D2PC_ERR_INVALID_ARG;
  if (!desc || desc->struct_size != sizeof(d2pc_score_filter_desc))
    return fail(ctx, D2PC_ERR_INVALID_ARG, "bad d2pc_score_filter_desc");
  const d2pc_score_filter_desc &d = *desc;
  if (d.direction != 0 && d.direction != 1) return fail(ctx, D2PC_ERR_INVALID_ARG, "direction %d is not 0 or 1", d.direction);
  if (d.form != D2PC_SCORE_FORM_CV4 && d.form != D2PC_SCORE_FORM_CV3)
    return fail(ctx, D2PC_ERR_INVALID_ARG, "unknown score form %d", d.form);
  if (d.width <= 0 || d.height <= 0 || d.n_frames <= 0 || d.n_frames > 65535)
    return fail(ctx, D2PC_ERR_BAD_SIZE, "bad size %dx%d x%d", d.width, d.height, d.n_frames);
  // the G21 halo (10 pixels) reflects once about the square's edges: n >= 11
  if (d.n < 11 || d.x < 0 || d.y < 0 || d.x > d.width - d.n || d.y > d.height - d.n)
    return fail(ctx, D2PC_ERR_BAD_SIZE, "square %d,%d,%d: n < 11 or outside %dx%d", d.x, d.y, d.n, d.width, d.height);
  if (!d.src || !d.out) return fail(ctx, D2PC_ERR_INVALID_ARG, "null device pointer");
  const int nf = d.n_frames;
  const Plane src{d.src, d.src_pitch, d.src_frame_stride, size_t(d.width), d.height};
  const Plane out{d.out, d.out_pitch, d.out_frame_stride, size_t(d.n), d.n};
  const Plane grad{d.grad, d.grad_pitch, d.grad_frame_stride, size_t(d.n), d.n};
  if (!src.fits(nf, Bound32::Plane))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "source pitch / frame stride too small (or plane >= 4 GiB)");
  if (!out.fits(nf, Bound32::Plane))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "out pitch / frame stride too small (or plane >= 4 GiB)");
  if (grad.p && !grad.fits(nf, Bound32::Plane))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "grad pitch / frame stride too small (or plane >= 4 GiB)");
  if (overlaps(src, out, nf) || overlaps(src, grad, nf))
    return fail(ctx, D2PC_ERR_INVALID_ARG, "an output overlaps the source (in-place filtering is not supported)");
  if (overlaps(out, grad, nf)) return fail(ctx, D2PC_ERR_INVALID_ARG, "out and grad overlap");
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  ScoreArgs a;
  a.src = static_cast<const uint8_t *>(d.src);
  a.out = static_cast<uint8_t *>(d.out);
  a.grad = static_cast<uint8_t *>(d.grad);
  a.src_pitch = uint32_t(d.src_pitch);
  a.out_pitch = uint32_t(d.out_pitch);
  a.grad_pitch = uint32_t(d.grad_pitch);
  a.src_frame_stride = src.kernel_frame_stride(nf);
  a.out_frame_stride = out.kernel_frame_stride(nf);
  a.grad_frame_stride = grad.kernel_frame_stride(nf);
  a.width = d.width, a.height = d.height, a.x0 = d.x, a.y0 = d.y, a.n = d.n, a.n_frames = d.n_frames;
  a.direction = d.direction;
  a.form = d.form;
  a.tile = ctx->score_tile;
  D2PC_HIP(ctx, launch_score_filter(a, static_cast<hipStream_t>(stream)));
  return D2PC_OK;
}

// ---------------------------------------------------------------------------
// colorizeDepth + the view of DisparityCb1/2 (src/depth_map_fusion.cpp:45-61,306-360)
// ---------------------------------------------------------------------------
int d2pc_colorize_table(uint8_t table[768]) {
  if (!table) return D2PC_ERR_INVALID_ARG;
  colorize_table(table);
  return D2PC_OK;
}

void d2pc_colorize_desc_init(d2pc_colorize_desc *desc) {
  if (!desc) return;
  memset(desc, 0, sizeof *desc);
  desc->struct_size = sizeof *desc;
  desc->rotate_cw = 0;
  desc->n_frames = 1;
}

int d2pc_colorize_device(d2pc_ctx *ctx, const d2pc_colorize_desc *desc, void *stream) {
  if (!ctx) return D2PC_ERR_INVALID_ARG;
  if (!desc || desc->struct_size != sizeof(d2pc_colorize_desc)) return fail(ctx, D2PC_ERR_INVALID_ARG, "bad d2pc_colorize_desc");
  const d2pc_colorize_desc &d = *desc;
  if (d.rotate_cw != 0 && d.rotate_cw != 1) return fail(ctx, D2PC_ERR_INVALID_ARG, "rotate_cw %d is not 0 or 1", d.rotate_cw);
  if (d.cols <= 0 || d.rows <= 0 || d.n_frames <= 0 || d.n_frames > 65535)
    return fail(ctx, D2PC_ERR_BAD_SIZE, "bad size %dx%d x%d", d.cols, d.rows, d.n_frames);
  // the frame the view is taken of: rotated, it has `cols` rows of `rows` pixels
  const int fw = d.rotate_cw ? d.rows : d.cols, fh = d.rotate_cw ? d.cols : d.rows;
  if (d.w <= 0 || d.h <= 0 || d.x < 0 || d.y < 0 || d.x > fw - d.w || d.y > fh - d.h)
    return fail(ctx, D2PC_ERR_BAD_SIZE, "view %d,%d %dx%d: empty or outside %dx%d", d.x, d.y, d.w, d.h, fw, fh);
  if (!d.src) return fail(ctx, D2PC_ERR_INVALID_ARG, "null device pointer");
  if (!d.gray && !d.rgb) return fail(ctx, D2PC_ERR_INVALID_ARG, "neither gray nor rgb output");
  const int nf = d.n_frames;
  const Plane src{d.src, d.src_pitch, d.src_frame_stride, size_t(d.cols), d.rows};
  const Plane gray{d.gray, d.gray_pitch, d.gray_frame_stride, size_t(d.w), d.h};
  const Plane rgb{d.rgb, d.rgb_pitch, d.rgb_frame_stride, 3 * size_t(d.w), d.h};
  if (!src.fits(nf, Bound32::Pitch)) return fail(ctx, D2PC_ERR_BAD_SIZE, "source pitch / frame stride too small");
  if (gray.p && !gray.fits(nf, Bound32::Pitch)) return fail(ctx, D2PC_ERR_BAD_SIZE, "gray pitch / frame stride too small");
  if (rgb.p && !rgb.fits(nf, Bound32::Pitch)) return fail(ctx, D2PC_ERR_BAD_SIZE, "rgb pitch (< 3 w) / frame stride too small");
  if (overlaps(src, gray, nf) || overlaps(src, rgb, nf))
    return fail(ctx, D2PC_ERR_INVALID_ARG, "an output overlaps the source");
  if (overlaps(gray, rgb, nf)) return fail(ctx, D2PC_ERR_INVALID_ARG, "gray and rgb overlap");
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  ColorizeArgs a;
  a.src = static_cast<const uint8_t *>(d.src);
  a.gray = static_cast<uint8_t *>(d.gray);
  a.rgb = static_cast<uint8_t *>(d.rgb);
  a.src_pitch = d.src_pitch, a.gray_pitch = d.gray_pitch, a.rgb_pitch = d.rgb_pitch;
  a.src_frame_stride = src.kernel_frame_stride(nf);
  a.gray_frame_stride = gray.kernel_frame_stride(nf);
  a.rgb_frame_stride = rgb.kernel_frame_stride(nf);
  a.cols = d.cols, a.rows = d.rows, a.x = d.x, a.y = d.y, a.w = d.w, a.h = d.h;
  a.n_frames = d.n_frames, a.rotate_cw = d.rotate_cw;
  D2PC_HIP(ctx, launch_colorize(a, static_cast<hipStream_t>(stream)));
  return D2PC_OK;
}

}  // extern "C"
