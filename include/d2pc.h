/*
 * d2pc.h -- C ABI of the MI355X-native disparity -> point-cloud path.
 *
 * Drop-in boundary for ONE path of PX4/disparity_to_point_cloud: the body of
 * d2pc::Disparity2PCloud::DisparityCb between
 *     real_disparity            (src/disparity_to_point_cloud.cpp:60-61)
 * and
 *     sensor_msgs::PointCloud2 output.data / width / ...   (cpp:84-85)
 * i.e. cv::reprojectImageTo3D (cpp:63-64) + the inset-40 ROI push_back loop
 * (cpp:70-76) + cloud metadata (cpp:79-81) + pcl::toROSMsg (cpp:84-85).
 * The reference has no FFI/plugin interface; a maintainer binds these entry
 * points from DisparityCb as shown in INTEGRATION.md.
 *
 * Plain C: pointers and sizes only.  No HIP, torch, ROS, OpenCV or PCL types.
 * Every function returns a d2pc_status (0 = OK) and never throws or aborts.
 * There is NO CPU fallback inside this library: without a usable gfx950
 * device d2pc_create() fails with D2PC_ERR_NO_DEVICE.
 *
 * Threading (mirrors the reference's single-threaded ros::spin(),
 * src/disparity_to_point_cloud_node.cpp:50): a context is not thread-safe;
 * distinct contexts (one per GPU / per camera stream) are independent.
 */
#ifndef D2PC_H
#define D2PC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version policy.  This header is the STABLE surface: what a maintainer binds from DisparityCb.
 * D2PC_ABI_VERSION changes when, and only when, a function here changes its signature or meaning, a struct here
 * changes its layout, an enumerator changes its value, or a symbol is removed; additions keep it (structs carry
 * struct_size / reserved fields for that).  d2pc_abi_version() returns the library's value: refuse a library whose
 * value differs from the header you compiled against.
 *   1  rounds 1-3: one header that also carried the bench / tuning / counter / graph-reservation entry points
 *   2  those moved to include/d2pc_ext.h (unstable: tools, tests and benchmarks only; no compatibility promise);
 *      the string keys that switched the arithmetic ("reproject_form", "force_general_q", "general_q_form") are gone
 *      from d2pc_set_tuning -- d2pc_set_reproject_form is the one way to choose the arithmetic */
#define D2PC_ABI_VERSION 2

typedef enum d2pc_status {
  D2PC_OK = 0,
  D2PC_ERR_INVALID_ARG = 1,   /* null pointer, bad struct_size, bad enum      */
  D2PC_ERR_BAD_DTYPE = 2,     /* dtype not one of D2PC_DTYPE_*                */
  D2PC_ERR_BAD_SIZE = 3,      /* width/height/stride out of range             */
  D2PC_ERR_CAPACITY = 4,      /* output buffer too small for the points       */
  D2PC_ERR_NO_DEVICE = 5,     /* no HIP device / device_id out of range       */
  D2PC_ERR_DEVICE = 6,        /* a HIP call failed (see d2pc_last_error)      */
  D2PC_ERR_NOT_CALIBRATED = 7,/* d2pc_set_q / d2pc_set_calibration not called */
  D2PC_ERR_OUT_OF_MEMORY = 8,
  D2PC_ERR_INTERNAL = 9       /* compaction hand-off timed out (bounded spin) */
} d2pc_status;

/* Sample type of the disparity image handed over.
 * F32 is the reference's `real_disparity` (CV_32FC1, cpp:60-61).
 * U8/U16 fuse the reference's convertTo(CV_32FC1, scale) (cpp:61) into the
 * kernel: d = (float)raw * scale in fp32 (scale = 1/8 in the reference). */
typedef enum d2pc_dtype {
  D2PC_DTYPE_F32 = 0,
  D2PC_DTYPE_U8 = 1,
  D2PC_DTYPE_U16 = 2,       /* raw 16-bit disparities, decoded as (float)v * scale                     */
  D2PC_DTYPE_MONO16 = 3     /* HOST entry points only (d2pc_process, d2pc_pipeline_*): a 16-bit image that
                               cv_bridge::toCvCopy(msg,"mono8") rescales to 8 bits first (cpp:50:
                               convertTo(CV_8U, 255./65535.)); the rescale runs on the device and the
                               frame continues as U8 (median allowed).  d2pc_process_mono16 = this. */
} d2pc_dtype;

typedef enum d2pc_mode {
  /* What the reference publishes (cpp:70-81): every ROI pixel, row-major,
   * nothing filtered (inf/NaN included), N = (W-2b)(H-2b), is_dense=false. */
  D2PC_MODE_PARITY = 0,
  /* Extension named by BASELINE.json's north_star: order-preserving removal
   * of points with a non-finite coordinate (or d <= min_disparity); the
   * survivors keep row-major order, so the cloud is dense (is_dense=true). */
  D2PC_MODE_COMPACT = 1
} d2pc_mode;

typedef struct d2pc_config {
  uint32_t struct_size;   /* = sizeof(d2pc_config); set by d2pc_config_init   */
  int32_t device_id;      /* HIP device ordinal (rank-local GPU)              */
  int32_t border;         /* ROI inset on all four sides; cpp:70,72 => 40     */
  int32_t mode;           /* d2pc_mode                                        */
  float min_disparity;    /* COMPACT only: also drop d <= this; -inf = off    */
  int32_t compact_algo;   /* 0 = library default: single pass (2) for launches
                             of >= 4 frames and >= ~20k tiles; one launch of
                             resident blocks (3) for launches of up to two 4K
                             frames that are not being captured; two-pass (1)
                             else.  1 = two-pass count/scan/scatter;
                             2 = single-pass counted hand-off; 3 = resident
                             blocks (falls back where impossible).  Same bytes
                             out whatever the value. */
  int32_t reserved[4];
} d2pc_config;

typedef struct d2pc_ctx d2pc_ctx;

/* sensor_msgs/PointCloud2 metadata that pcl::toROSMsg (cpp:84-85) fills for a
 * pcl::PointCloud<pcl::PointXYZ> of n points with cpp:79-81's width/height. */
typedef struct d2pc_field { char name[8]; uint32_t offset; uint8_t datatype; uint32_t count; } d2pc_field;
typedef struct d2pc_cloud_meta {
  uint32_t height;        /* 1  (cpp:80)                                      */
  uint32_t width;         /* n  (cpp:79)                                      */
  uint32_t point_step;    /* 16 = sizeof(pcl::PointXYZ)                       */
  uint32_t row_step;      /* 16*n                                             */
  uint8_t is_bigendian;   /* 0                                                */
  uint8_t is_dense;       /* 0 in PARITY (cpp:81), 1 in COMPACT               */
  uint32_t n_fields;      /* 3                                                */
  d2pc_field fields[3];   /* x,y,z FLOAT32(7) @ 0,4,8 count 1                 */
} d2pc_cloud_meta;

/* Calibration blob broadcast once from rank 0 to every GPU's process
 * (RCCL/xGMI broadcast in the multi-GPU harness): 16 x f64 Q + border + mode. */
#define D2PC_CALIB_BLOB_BYTES 136

/* ---- library-level ---------------------------------------------------- */
int d2pc_abi_version(void);
const char *d2pc_status_string(int status);
int d2pc_device_count(void);            /* number of HIP devices, 0 if none  */

/* ---- calibration surface (hpp:66-71,84-104) --------------------------- */
/* Closed form of the reference's cv::stereoRectify call for its rig
 * (identical pinhole cameras, zero distortion, R = I, t = (-baseline,0,0),
 * image size (nx,ny) = (752,480) at hpp:101-103).  Host-only helper for
 * ROS-free callers; the ROS adaptor passes OpenCV's own Q_ to d2pc_set_q.
 * d2pc_make_q = D2PC_STEREORECTIFY_CONTINUOUS below. */
int d2pc_make_q(double fx, double fy, double cx, double cy, double baseline,
                int nx, int ny, double q_out[16]);

/* Where stereoRectify puts the new principal point depends on the OpenCV
 * release (the image-corner coordinates and the centre it re-centres on
 * changed between 2.4 and 3.x), and the reference pins no version.  For the
 * reference's case (no distortion, R = I) with c = source principal point,
 * n = image extent, f' = fy:
 *   CONTINUOUS  c' = (n-1)/2.0 - f'((n-1)/2.0 - c)/f   SURVEY.md section 8 row a9; no release computes
 *               exactly this (real-valued centre), it is "this closed form"
 *   CV24        c' = n/2 - f'(n/2.0 - c)/f     OpenCV 2.4.x (ROS Indigo, what .clang_complete:2 points at):
 *               corners at 0 and n, integer n/2.  752x480 defaults: cx' = 376 exactly
 *   CV3         c' = (n-1)/2 - f'((n-1)/2.0 - c)/f   OpenCV 3.x/4.x: corners at 0 and n-1, INTEGER (n-1)/2.
 *               752x480 defaults: cx' = 375.4995...
 * OpenCV evaluates parts of this in float, so none of the three is bit-for-bit
 * a release's Q: a node that has OpenCV passes ITS Q to d2pc_set_q
 * (ros/disparity_to_point_cloud_node.cpp does); the host mirror without OpenCV
 * defaults to CV24. */
typedef enum d2pc_stereorectify_flavour {
  D2PC_STEREORECTIFY_CONTINUOUS = 0,
  D2PC_STEREORECTIFY_CV24 = 1,
  D2PC_STEREORECTIFY_CV3 = 2
} d2pc_stereorectify_flavour;
int d2pc_make_q_flavour(double fx, double fy, double cx, double cy, double baseline,
                        int nx, int ny, int flavour, double q_out[16]);

/* Q for a stereo_msgs/DisparityImage-style source (SURVEY.md section 8(f) #3:
 * calibration carried by the message instead of ~fx_.. parameters): focal
 * length f (pixels), baseline T (metres, > 0), principal point (cx, cy):
 *   Q = [1 0 0 -cx; 0 1 0 -cy; 0 0 0 f; 0 0 1/T 0]  =>  Z = f*T/d. */
int d2pc_make_q_disparity_image(double f, double T, double cx, double cy, double q_out[16]);

/* Host-only packing of the calibration blob (what rank 0 broadcasts): usable
 * without a device, e.g. by the process that owns the ROS parameters. */
int d2pc_calib_pack(const double q[16], int border, int mode, void *blob /*136 B*/);
int d2pc_calib_unpack(const void *blob, size_t blob_bytes, double q_out[16], int *border, int *mode);

/* ---- context ---------------------------------------------------------- */
int d2pc_config_init(d2pc_config *cfg); /* reference defaults: border 40, PARITY */
int d2pc_create(const d2pc_config *cfg, d2pc_ctx **out_ctx);
int d2pc_destroy(d2pc_ctx *ctx);
const char *d2pc_last_error(const d2pc_ctx *ctx);

/* Q_ (hpp:72), row-major 4x4 doubles exactly as Q_.ptr<double>() yields. */
int d2pc_set_q(d2pc_ctx *ctx, const double q[16]);
int d2pc_get_q(const d2pc_ctx *ctx, double q_out[16]);
int d2pc_set_border(d2pc_ctx *ctx, int border);
int d2pc_set_mode(d2pc_ctx *ctx, int mode);
/* Which cv::reprojectImageTo3D (cpp:64) the points reproduce.  The two OpenCV
 * generations evaluate the same Q*[x y d 1]^T in different orders and differ
 * from each other by up to 1 float ulp (more where a numerator cancels):
 *   D2PC_FORM_DEFAULT  cv::stereoRectify's Q: a specialised kernel, <= 1 ulp
 *                      from BOTH generations (the exact quotient rounded once);
 *                      any other Q: OpenCV 3/4's form bit for bit
 *   D2PC_FORM_CV24     OpenCV 2.4's loop bit for bit (per row qx = q01*y + q03,
 *                      then qx += q00 per column, one rounding per step).  That
 *                      recurrence is sequential in x; it is reproduced in
 *                      parallel only for a Q whose column steps are exact
 *                      (q00 = 1, q01 = q10 = q20 = q30 = +0 -- what
 *                      stereoRectify and d2pc_make_q* produce); any other Q
 *                      makes the next call return D2PC_ERR_INVALID_ARG.  The
 *                      running sum rounds once per binade it crosses inside a
 *                      row; the library holds 18 such segments (a principal
 *                      point of any size on rows of up to 65,536 columns) and
 *                      returns D2PC_ERR_BAD_SIZE beyond
 *   D2PC_FORM_CV4      OpenCV 3/4's form bit for bit for every Q (Matx product
 *                      left to right, numerators cast to float, times 1./W)
 * For cv::stereoRectify's Q the exact forms have kernels of their own and cost
 * about as much as the default; any other Q runs them in the general kernel
 * (double, no contraction), which is arithmetic-bound:
 * profiles/r03_ab_forms.txt has all of them beside the default. */
typedef enum d2pc_reproject_form {
  D2PC_FORM_DEFAULT = 0,
  D2PC_FORM_CV24 = 24,
  D2PC_FORM_CV4 = 4
} d2pc_reproject_form;
int d2pc_set_reproject_form(d2pc_ctx *ctx, int form);
/* COMPACT predicate threshold (e.g. DisparityImage.min_disparity): points with
 * d <= min_disparity are dropped; -inf disables it.  NaN is rejected. */
int d2pc_set_min_disparity(d2pc_ctx *ctx, float min_disparity);
int d2pc_get_config(const d2pc_ctx *ctx, d2pc_config *cfg_out);
int d2pc_export_calibration(const d2pc_ctx *ctx, void *blob /*136 B*/);
int d2pc_import_calibration(d2pc_ctx *ctx, const void *blob, size_t blob_bytes);

/* Number of ROI pixels (= points in PARITY mode): max(w-2b,0)*max(h-2b,0). */
size_t d2pc_roi_points(int width, int height, int border);
int d2pc_cloud_meta_fill(const d2pc_ctx *ctx, size_t n_points, d2pc_cloud_meta *meta);

/* ---- the hot path ----------------------------------------------------- */
/*
 * Replaces cpp:63-85 for one frame held in HOST memory (synchronous).
 *   disp              H x W samples of `dtype`, rows `row_stride_bytes` apart
 *   scale             U8/U16 only (cpp:61: 1/8); ignored for F32
 *   out_points        capacity_points records of 16 bytes {x,y,z,1.0f}: the
 *                     exact bytes of PointCloud2.data (pass output.data.data())
 *   out_index         nullable; source pixel index v*W+u of every emitted
 *                     point (uint32)
 *   n_points          points written: (W-2b)(H-2b) in PARITY, #valid in COMPACT
 * Nothing is retained after return.
 */
int d2pc_process(d2pc_ctx *ctx, const void *disp, int dtype, float scale,
                 int width, int height, size_t row_stride_bytes,
                 void *out_points, uint32_t *out_index,
                 size_t capacity_points, size_t *n_points);

/*
 * Device-resident, batched, asynchronous form (frames already in HBM):
 * n_frames frames, `in_frame_stride_bytes` apart, are converted by ONE
 * kernel sequence enqueued on `stream` (a hipStream_t passed as void*;
 * NULL = HIP's default stream, as in the HIP API).  Frame f's points go to
 * d_out_points + f*out_frame_stride_points*16 (and d_out_index +
 * f*out_frame_stride_points); d_counts[f] (uint32, nullable in PARITY)
 * receives the number of points of frame f.  All device pointers must belong
 * to the context's device; d_out_points must be 16-byte aligned -- 128-byte
 * alignment (of the base and of out_frame_stride_points*16) keeps every wave
 * store on whole 64-byte memory requests (a base that is only 16-byte aligned is slower).
 * Does not synchronise.
 *
 * COMPACT launches in flight at once: calls on ONE stream are ordered and share
 * the context's compaction state; a call on another stream gets a state buffer
 * of its own (up to 8 per context), so double-buffered use of one context on
 * two streams is safe.  The context itself is still used from one host thread.
 * A stream handed to a COMPACT call (here and in d2pc_process_mono_device) must
 * stay valid until the context is destroyed: the context asks it later whether
 * the work it was given has drained, before another stream may take the buffer.
 *
 * hipGraph capture: nothing can be allocated while capturing, so a COMPACT call
 * needs its state buffer beforehand (D2PC_ERR_OUT_OF_MEMORY otherwise): run the
 * largest batch once, or reserve it (d2pc_reserve in d2pc_ext.h) before EACH
 * capture.  The state buffer a capture used belongs to that graph from then on:
 * later calls never free, grow or share it, so the graph stays replayable
 * whatever else the context is asked to do (d2pc_release_graph_buffers in
 * d2pc_ext.h hands them back).  One replay of a given graph in flight at a time.
 *
 * COMPACT failure reporting in-band: if the single-pass kernel gave up waiting
 * for an earlier tile (see d2pc_check_async_error) d_counts[f] of the affected
 * frames is 0xFFFFFFFF instead of a count.
 */
int d2pc_process_device(d2pc_ctx *ctx, const void *d_disp, int dtype,
                        float scale, int width, int height,
                        size_t row_stride_bytes, size_t in_frame_stride_bytes,
                        int n_frames, void *d_out_points,
                        uint32_t *d_out_index,
                        size_t out_frame_stride_points, uint32_t *d_counts,
                        void *stream);

/*
 * The rest of the callback body on the device:
 * k x k median of 8-bit frames with replicated borders, i.e.
 * cv::medianBlur(image, filtered, 11) at cpp:55-57.  ksize odd, 3..11.
 * Device-resident, batched, asynchronous on `stream` like
 * d2pc_process_device; src and dst must not overlap.
 */
int d2pc_median_device(d2pc_ctx *ctx, const void *d_src, int width, int height,
                       size_t src_row_stride_bytes, size_t src_frame_stride_bytes,
                       int n_frames, void *d_dst, size_t dst_row_stride_bytes,
                       size_t dst_frame_stride_bytes, int ksize, void *stream);

/*
 * The same filter restricted to what the callback reads afterwards: only the
 * pixels of the context's inset ROI (cpp:70,72: rows and columns [border,
 * dim - border)) are computed and written; d_dst outside the ROI is left
 * untouched.  Windows still read the whole source image (replicated only at
 * its true edges), so every ROI pixel equals d2pc_median_device's.  At the
 * reference's 752x480 / border 40 this is 25.5 % less work.  The fused entry
 * points (d2pc_process_mono8/16, d2pc_pipeline_*) filter this way.
 */
int d2pc_median_roi_device(d2pc_ctx *ctx, const void *d_src, int width, int height,
                       size_t src_row_stride_bytes, size_t src_frame_stride_bytes,
                       int n_frames, void *d_dst, size_t dst_row_stride_bytes,
                       size_t dst_frame_stride_bytes, int ksize, void *stream);

/*
 * cv_bridge::toCvCopy(msg, "mono8") applied to a mono16 image (cpp:50) on the
 * device: dst = saturate(round_half_even(src * (float)(255./65535.))), i.e.
 * cv::Mat::convertTo(CV_8U, 255./65535.).  src rows hold uint16 samples (strides
 * in bytes, 2-byte aligned); asynchronous on `stream`; src and dst must not overlap.
 */
int d2pc_mono16_to_mono8_device(d2pc_ctx *ctx, const void *d_src, int width, int height,
                                size_t src_row_stride_bytes, size_t src_frame_stride_bytes,
                                int n_frames, void *d_dst, size_t dst_row_stride_bytes,
                                size_t dst_frame_stride_bytes, void *stream);

/*
 * cpp:55-85 in one call for one mono8 frame in HOST memory (what
 * cv_bridge::toCvCopy(msg,"mono8") returned, cpp:50): median (median_ksize,
 * the reference uses 11; 0 or 1 = none) -> x scale (1/8, cpp:61) ->
 * reprojection + ROI pack.  Only 1 byte per pixel crosses PCIe on the way in.
 * Other arguments as d2pc_process.
 */
int d2pc_process_mono8(d2pc_ctx *ctx, const uint8_t *image, int width, int height,
                       size_t row_stride_bytes, int median_ksize, float scale,
                       void *out_points, uint32_t *out_index,
                       size_t capacity_points, size_t *n_points);

/* The same for a mono16 frame (what the node receives when the disparity is
 * published as 16-bit): cpp:50's cv_bridge rescale to mono8 runs on the device
 * in front of the median.  2 bytes per pixel cross PCIe on the way in. */
int d2pc_process_mono16(d2pc_ctx *ctx, const uint16_t *image, int width, int height,
                        size_t row_stride_bytes, int median_ksize, float scale,
                        void *out_points, uint32_t *out_index,
                        size_t capacity_points, size_t *n_points);

/*
 * The whole callback body (cpp:50-85) for a BATCH of frames resident in HBM:
 * [MONO16: cv_bridge rescale ->] k x k median over the inset ROI -> x scale ->
 * reproject + pack, asynchronous on `stream` like d2pc_process_device (same
 * output arguments).  dtype is D2PC_DTYPE_U8 or D2PC_DTYPE_MONO16;
 * median_ksize 0/1 skips the filter.
 *
 * With the default tuning, PARITY mode and a launch of at least 448 tiles of
 * 256 x 32 ROI pixels (one 4K frame has 975; 192 / 320 tiles for 3x3 / 5x5 windows) the call is ONE
 * kernel that works tile by tile: the bit-sliced median of the tile, then the
 * tile's points straight from the filtered bytes in LDS -- for stereoRectify's Q
 * through a per-block table of 1/W and Z over the 256 byte values.  The filtered
 * frames never reach memory.  Everything else -- small launches -- is the filter
 * launch followed by the reprojection launch.  The results are the same bytes
 * either way (measurements: DESIGN.md section 5).
 * (Launch-shape knobs: d2pc_set_tuning in d2pc_ext.h.)
 * In the two-launch form the filtered frames live in a scratch buffer that belongs
 * to the calling stream's work (one per stream in flight, like the compaction
 * state: double-buffered use on two streams is safe); it is grown on demand, so
 * before a capture run the batch size once (or reserve it: d2pc_reserve_mono in
 * d2pc_ext.h); under stream capture the call runs in order on `stream`.  The
 * one-kernel form needs no scratch.
 */
int d2pc_process_mono_device(d2pc_ctx *ctx, const void *d_image, int dtype, int width, int height,
                             size_t row_stride_bytes, size_t frame_stride_bytes, int n_frames,
                             int median_ksize, float scale, void *d_out_points, uint32_t *d_out_index,
                             size_t out_frame_stride_points, uint32_t *d_counts, void *stream);

/*
 * Pinned (page-locked) host buffers for the synchronous entry points above
 * ("write the output into a pinned buffer that IS
 * output.data").  When `out_points` (and `out_index`, if given) of a
 * d2pc_process* call lie in memory from d2pc_host_alloc and hold the whole ROI
 * (capacity_points >= ROI points), the kernels store the final PointCloud2
 * bytes straight into it over PCIe: no device-side copy of the cloud, no
 * D2H copy, no bounce through the runtime's staging buffers.  A pinned `disp`
 * / `image` is read by the reprojection kernel in place when that kernel is the
 * first to touch it (PARITY, no median, no mono16 rescale: the inbound reads
 * then overlap the outbound stores on the full-duplex link); otherwise it makes
 * the upload one DMA.  Pageable buffers keep working as before.
 * host/pinned_allocator.hpp wraps these two in a caching std::allocator so that
 * sensor_msgs::PointCloud2_<Alloc>::data can be such a buffer.
 */
void *d2pc_host_alloc(size_t bytes);
void d2pc_host_free(void *p);

/*
 * Pipelined host path: up to `depth`
 * frames in flight, each on its own HIP stream with its own PINNED staging:
 *   acquire -> the caller decodes the image straight into pinned memory
 *   submit  -> async H2D, (median), kernels, D2H (or, with direct_host_write,
 *              the kernels store the points straight into pinned host memory)
 *   collect -> waits for the OLDEST submitted frame and hands out a view of
 *              its pinned output: the PointCloud2 payload without another copy
 *   release -> the slot can be acquired again
 * The copy in of frame i+1, the kernels of frame i and the copy out of frame
 * i-1 overlap.  Frames are collected in submission order.
 */
typedef struct d2pc_frame_desc {
  int32_t dtype;             /* d2pc_dtype (MONO16 allowed) */
  float scale;               /* U8/U16 decode scale (cpp:61: 1/8) */
  int32_t width, height;
  size_t row_stride_bytes;   /* layout of the pinned input buffer */
  int32_t median_ksize;      /* 0/1 = none; else odd 3..11, U8 only (cpp:55-57) */
  int32_t want_index;        /* also produce source pixel indices */
  uint64_t tag;              /* returned by collect (e.g. the message stamp) */
} d2pc_frame_desc;

int d2pc_pipeline_configure(d2pc_ctx *ctx, int depth /*1..8*/, int direct_host_write);
int d2pc_pipeline_acquire(d2pc_ctx *ctx, const d2pc_frame_desc *desc, void **host_in, int *slot);
int d2pc_pipeline_submit(d2pc_ctx *ctx, int slot);
int d2pc_pipeline_collect(d2pc_ctx *ctx, int *slot, const void **points, const uint32_t **index,
                          size_t *n_points, uint64_t *tag);
int d2pc_pipeline_release(d2pc_ctx *ctx, int slot);

/* After the streams of the context's COMPACT d2pc_process_device calls have been
 * synchronised: D2PC_ERR_INTERNAL if a hand-off wait of the single-pass kernel
 * ran out of its time budget (4 s) in the
 * LAST launch of any of the context's state buffers -- each buffer remembers
 * the algorithm of its own last launch.  The output of such a launch is
 * incomplete and its d_counts entries read 0xFFFFFFFF; relaunch with
 * compact_algo = 1.  d2pc_process* (synchronous) does that relaunch itself;
 * d2pc_pipeline_collect reports the frame as D2PC_ERR_INTERNAL. */
int d2pc_check_async_error(d2pc_ctx *ctx);

/*
 * SURVEY.md section 8(f) #4 -- the inner loop of the sibling node's
 * DepthMapFusion::publishFusedDepthMap, device-resident and batched:
 *   per pixel  fused = rule(depth1, depth2, score1, score2, grad1, grad2)
 *              (src/depth_map_fusion.cpp:115-117,150-160; rules :162-235),
 *              combined = min(grad1, grad2)                  (:118-121)
 *   then       cv::medianBlur(fused, fused, 3)               (:124)
 *   then       cropMat(fused, left, right, top, bottom)      (:130: 0,40,30,10)
 * in one kernel.  Rules are numbered in the reference's source order;
 * GRAD_FILTER is the one getFusedDistance calls (:159).  WEIGHTED_AVERAGE
 * divides by zero in the reference when both scores are non-zero; that case
 * is defined as 0 here.
 */
typedef enum d2pc_fusion_rule {
  D2PC_FUSE_WEIGHTED_AVERAGE = 0,
  D2PC_FUSE_MAX_DIST = 1,
  D2PC_FUSE_MAX_DIST_UNLESS_BLACK = 2,
  D2PC_FUSE_BETTER_SCORE = 3,
  D2PC_FUSE_ONLY_GOOD_1 = 4,
  D2PC_FUSE_ONLY_GOOD_AVG = 5,
  D2PC_FUSE_OVERLAP = 6,
  D2PC_FUSE_BLACK_TO_WHITE = 7,
  D2PC_FUSE_GRAD_FILTER = 8
} d2pc_fusion_rule;

typedef struct d2pc_fuse_desc {
  uint32_t struct_size;        /* sizeof(d2pc_fuse_desc) */
  int32_t rule;                /* d2pc_fusion_rule */
  int32_t width, height;       /* of every input plane (n x n after cropToSquare in the reference) */
  int32_t n_frames;            /* independent plane sets, frame_stride apart */
  int32_t crop_left, crop_right, crop_top, crop_bottom;
  const void *planes[6];       /* DEVICE: depth1, depth2, score1, score2, grad1, grad2 (8-bit).
                                  grad1/grad2 may be NULL when `combined` is NULL; planes may alias each
                                  other (the reference's score1 and grad1 share a buffer, cpp:77) */
  size_t pitch[6];             /* bytes between rows */
  size_t frame_stride[6];      /* bytes between frames (ignored when n_frames == 1) */
  void *fused;                 /* DEVICE out: (width-left-right) x (height-top-bottom) */
  size_t fused_pitch, fused_frame_stride;
  void *combined;              /* DEVICE out, nullable: width x height */
  size_t combined_pitch, combined_frame_stride;
} d2pc_fuse_desc;

/* struct_size, GRAD_FILTER, n_frames 1, crop 0/40/30/10; everything else zero. */
void d2pc_fuse_desc_init(d2pc_fuse_desc *desc);
/* Asynchronous on `stream` (NULL = the HIP default stream).  Outputs must not
 * overlap the inputs or each other: the reference writes `combined` over
 * score1 in place (cpp:113), which a caller reproduces by swapping buffers
 * (the Python FusionNode session does). */
int d2pc_fuse_device(d2pc_ctx *ctx, const d2pc_fuse_desc *desc, void *stream);
/* rotateMat (src/depth_map_fusion.cpp:268-273: cv::transpose + cv::flip(.,1) = 90 degrees clockwise) of 8-bit
 * frames on the device: dst has `cols` rows of `rows` pixels, dst(i,j) = src(rows-1-j, i).  What DisparityCb2 and
 * MatchingScoreCb2 apply to camera 2's images before cropToSquare (cpp:56,84).  Asynchronous on `stream`. */
int d2pc_rotate_cw_device(d2pc_ctx *ctx, const void *d_src, int cols, int rows, size_t src_pitch,
                          size_t src_frame_stride, int n_frames, void *d_dst, size_t dst_pitch,
                          size_t dst_frame_stride, void *stream);
/* cropToSquare (src/depth_map_fusion.cpp:247-265): the square view of a
 * cols x rows image, shifted by the offsets.  The side length uses the class
 * member offset_y_ (cpp:253), the origin the argument: pass both. */
int d2pc_crop_to_square(int cols, int rows, int offset_x, int offset_y, int member_offset_y,
                        int *x, int *y, int *n);

/*
 * The matching-score pre-filter of MatchingScoreCb1/2 (src/depth_map_fusion.cpp:64-99) on the device:
 *   A   = GaussianBlur(square, 13x13, 3)                 (:70,:89)  the square is a VIEW (cropToSquare, :66,:85):
 *                                                                   the blur reads the frame's pixels round it and
 *                                                                   reflects (reflect101) only about the FRAME's edges
 *   M   = threshold(Sobel(A, -1, dx, dy, 7, 0.03), 30)   (:72-73,:91-92)  direction 0: (0,2), 1: (2,0);
 *                                                                   reflect101 about the square's edges
 *   B   = GaussianBlur(M, 21x21, 10)                     (:74,:93)  reflect101 about the square's edges
 *   out = square + 2 * B, saturated                      (:76,:95)  what the reference keeps as both the score
 *                                                                   and the grad plane (:77,:96)
 * in exact integers.  The two forms differ only in B: D2PC_SCORE_FORM_CV4 takes OpenCV 4.x's
 * bit-exact fixed-point Gaussian (taps sum 256, rounds half up), D2PC_SCORE_FORM_CV3 OpenCV 3.2's general 8-bit
 * path (taps sum 254, rounds half to even).  A is the same in both (general path: a view is never bit-exact).
 */
typedef enum d2pc_score_form { D2PC_SCORE_FORM_CV4 = 4, D2PC_SCORE_FORM_CV3 = 3 } d2pc_score_form;

typedef struct d2pc_score_filter_desc {
  uint32_t struct_size;        /* sizeof(d2pc_score_filter_desc) */
  int32_t direction;           /* 0: Sobel(0,2) of MatchingScoreCb1, 1: Sobel(2,0) of MatchingScoreCb2 */
  int32_t form;                /* d2pc_score_form */
  int32_t width, height;       /* of the source frames (camera 2: already rotated, d2pc_rotate_cw_device) */
  int32_t n_frames;            /* independent frames, frame strides apart */
  int32_t x, y, n;             /* the square (d2pc_crop_to_square); n >= 11 */
  const void *src;             /* DEVICE: 8-bit frames */
  size_t src_pitch, src_frame_stride;
  void *out;                   /* DEVICE out: n x n, min(255, score + 2 B) */
  size_t out_pitch, out_frame_stride;
  void *grad;                  /* DEVICE out, nullable: n x n, B (before the combine) */
  size_t grad_pitch, grad_frame_stride;
} d2pc_score_filter_desc;

/* struct_size, direction 0, D2PC_SCORE_FORM_CV4, n_frames 1; everything else zero. */
void d2pc_score_filter_desc_init(d2pc_score_filter_desc *desc);
/* Asynchronous on `stream` (NULL = the HIP default stream).  Outputs must not overlap the source or each other
 * (no in-place filtering). */
int d2pc_score_filter_device(d2pc_ctx *ctx, const d2pc_score_filter_desc *desc, void *stream);

/*
 * colorizeDepth (src/depth_map_fusion.cpp:306-360): the RAINBOW_WITH_BLACK colouring of the /cropped_depth_1,
 * /cropped_depth_2 and /gradient topics.  A function of the 8-bit pixel alone, so a 256 x 3 table (DESIGN.md
 * section 8b): row g is bytes 3g .. 3g+2 in MEMORY order (the reference names them b, g, r and publishes the buffer
 * as "rgb8").  Computed on the host in IEEE float32, one rounding per operation; rows 0 and 1 are black.
 * Host only: no context, no GPU.  Returns D2PC_OK, or D2PC_ERR_INVALID_ARG for NULL.
 */
int d2pc_colorize_table(uint8_t table[768]);

/*
 * The body of DisparityCb1 / DisparityCb2 (:45-61) and of the /gradient publish (:132) in one launch: take a w x h
 * view of each 8-bit frame -- optionally of the frame rotated 90 degrees clockwise, as d2pc_rotate_cw_device
 * defines it (dst(i,j) = src(rows-1-j, i)), WITHOUT materialising the rotated frame -- and write the view itself
 * (`gray`, the reference's cropped_depth_k_) and / or its colouring (`rgb`, w x h x 3 bytes).  Neither output needs
 * any alignment: a packed rgb image has pitch 3w, odd for odd w.
 */
typedef struct d2pc_colorize_desc {
  uint32_t struct_size;        /* sizeof(d2pc_colorize_desc) */
  int32_t rotate_cw;           /* 0: view of the frame; 1: view of the frame rotated 90 degrees clockwise */
  int32_t cols, rows;          /* of the source frames as stored (before the rotation) */
  int32_t n_frames;            /* independent frames, frame strides apart */
  int32_t x, y, w, h;          /* the view, in the (rotated) frame's coordinates: what d2pc_crop_to_square returns,
                                  or 0, 0 and the whole (rotated) plane */
  const void *src;             /* DEVICE: 8-bit frames */
  size_t src_pitch, src_frame_stride;
  void *gray;                  /* DEVICE out, nullable: w x h, the view copied */
  size_t gray_pitch, gray_frame_stride;
  void *rgb;                   /* DEVICE out, nullable: w x h x 3 bytes, pitch >= 3 w */
  size_t rgb_pitch, rgb_frame_stride;
} d2pc_colorize_desc;

/* struct_size, rotate_cw 0, n_frames 1; everything else zero. */
void d2pc_colorize_desc_init(d2pc_colorize_desc *desc);
/* Asynchronous on `stream` (NULL = the HIP default stream); no scratch memory, so it can be captured into a graph
 * as it is.  At least one output; outputs must not overlap the source or each other. */
int d2pc_colorize_device(d2pc_ctx *ctx, const d2pc_colorize_desc *desc, void *stream);

/*
 * The depth_map_fusion node (src/depth_map_fusion.cpp) as a SESSION: the four callbacks, the state they share and the
 * seven topics they publish, for `batch` independent camera pairs.  The node owns every plane on its context's device
 * (two depth planes, camera 1's score plane and a spare, camera 2's score plane and its rotated frame, two colour
 * images, the fused map and its colouring); everything is allocated by d2pc_fusion_node_create, so a callback is a
 * fixed sequence of kernel launches: no allocation, no device-to-device copy.
 *
 * The reference keeps camera 1's score, its grad and the combined confidence in ONE buffer (:77,:113): each fusion
 * leaves min(grad1, grad2) in camera 1's score plane until the next matching-score-1 callback, and a disparity-2
 * callback without new scores fuses against that.  The node reproduces this by swapping the score plane with the
 * spare, never by copying; which is which is HOST state.  So the COMBINED_SCORE and CROPPED_SCORE_1 buffers are
 * additionally overwritten by the next MATCHING_SCORE_1 / DISPARITY_2 callback; every other topic's buffer by the next
 * callback that publishes that topic.
 */
typedef enum d2pc_fusion_node_callback_id {
  D2PC_NODE_DISPARITY_1 = 0,        /* DisparityCb1 (:45-51)      publishes CROPPED_DEPTH_1 */
  D2PC_NODE_DISPARITY_2 = 1,        /* DisparityCb2 (:53-61)      CROPPED_DEPTH_2 and, once all four planes have arrived
                                       (:106-109), COMBINED_SCORE, GRADIENT, FUSED_DEPTH_MAP */
  D2PC_NODE_MATCHING_SCORE_1 = 2,   /* MatchingScoreCb1 (:64-80)  CROPPED_SCORE_1 */
  D2PC_NODE_MATCHING_SCORE_2 = 3    /* MatchingScoreCb2 (:82-99)  CROPPED_SCORE_2 */
} d2pc_fusion_node_callback_id;

/* Topics, in the order of the reference's publishers; bit (1 << id) of a `published` mask. */
typedef enum d2pc_fusion_node_topic_id {
  D2PC_TOPIC_CROPPED_DEPTH_1 = 0,   /* n x n x 3 */
  D2PC_TOPIC_CROPPED_DEPTH_2 = 1,   /* n x n x 3 */
  D2PC_TOPIC_CROPPED_SCORE_1 = 2,   /* n x n */
  D2PC_TOPIC_CROPPED_SCORE_2 = 3,   /* n x n */
  D2PC_TOPIC_FUSED_DEPTH_MAP = 4,   /* fused_width x fused_height */
  D2PC_TOPIC_COMBINED_SCORE = 5,    /* n x n */
  D2PC_TOPIC_GRADIENT = 6           /* fused_width x fused_height x 3 */
} d2pc_fusion_node_topic_id;
#define D2PC_NODE_TOPICS 7

typedef struct d2pc_fusion_node_config {
  uint32_t struct_size;        /* sizeof(d2pc_fusion_node_config) */
  int32_t cols, rows;          /* of every incoming frame */
  int32_t offset_x, offset_y;  /* the node's params (:119-124) */
  int32_t rule;                /* d2pc_fusion_rule */
  int32_t score_form;          /* d2pc_score_form */
  int32_t batch;               /* independent camera pairs per callback */
  int32_t crop_left, crop_right, crop_top, crop_bottom;   /* cropMat of publishFusedDepthMap (:130) */
  int32_t single_launch;       /* 1: a fusing DISPARITY_2 with rule GRAD_FILTER is ONE kernel launch; 0: always the
                                  three-launch composition.  Same bytes either way.  One launch is 3 x faster for one
                                  camera frame, level at 16 and slower beyond: large batches set 0. */
  int32_t reserved[3];
} d2pc_fusion_node_config;

/* struct_size; offsets 0/0 (the class defaults, hpp:92-93); GRAD_FILTER (:159); D2PC_SCORE_FORM_CV4; batch 1; crop
 * 0/40/30/10 (:130); single_launch 1; cols = rows = 0: the caller's to set. */
void d2pc_fusion_node_config_init(d2pc_fusion_node_config *cfg);

typedef struct d2pc_fusion_node_geometry_t {
  int32_t x1, y1;              /* camera 1's square: cropToSquare(frame, offset_x, offset_y) */
  int32_t x2, y2;              /* camera 2's, in the ROTATED frame: cropToSquare(rotated, -offset_x, -offset_y), its
                                  side from the member offset_y (:253) */
  int32_t n;                   /* side of both */
  int32_t fused_width, fused_height;
  int32_t reserved;
  size_t topic_bytes[D2PC_NODE_TOPICS];  /* bytes of each topic's image, all `batch` pairs together */
} d2pc_fusion_node_geometry_t;

/* Host arithmetic only (no context, no device).  D2PC_ERR_BAD_SIZE when a square leaves its frame, the two squares
 * differ in size, n < 11 (the score filter's halo) or the crop leaves nothing of the fused map -- and when
 * |offset_x| > |offset_y|: there the reference re-crops the frame it fuses into with a side of min(cols, rows) -
 * |offset_y| (:106, :253) but fuses only min(cols, rows) - max(|offset_x|, |offset_y|) of it, and publishes a larger
 * fused map with a margin of raw camera-2 pixels.  That is not reproduced. */
int d2pc_fusion_node_geometry(const d2pc_fusion_node_config *cfg, d2pc_fusion_node_geometry_t *out);

typedef struct d2pc_fusion_node d2pc_fusion_node;
/* The node lives on `ctx`'s device and must be destroyed before the context. */
int d2pc_fusion_node_create(d2pc_ctx *ctx, const d2pc_fusion_node_config *cfg, d2pc_fusion_node **out);
int d2pc_fusion_node_destroy(d2pc_fusion_node *node);

typedef struct d2pc_fusion_node_topic {
  void *data;                  /* DEVICE: the node's own buffer */
  size_t pitch, frame_stride;  /* bytes between rows / between the pairs of a batch */
  int32_t width, height, channels, reserved;
} d2pc_fusion_node_topic;
typedef struct d2pc_fusion_node_topics {
  uint32_t struct_size;        /* sizeof(d2pc_fusion_node_topics), set by the caller */
  uint32_t published;          /* out: bit (1 << d2pc_fusion_node_topic_id) per topic this call published */
  d2pc_fusion_node_topic topic[D2PC_NODE_TOPICS];  /* out: filled for the published topics, zero otherwise */
} d2pc_fusion_node_topics;

/* One callback on frames resident on the device: `batch` mono8 frames of cols x rows, `frame_stride` bytes apart
 * (ignored for batch 1), rows `pitch` bytes apart.  Asynchronous on `stream` (NULL = the HIP default stream).
 * Capturable into a graph; a captured callback is pinned to the planes it was captured with, so capture
 * MATCHING_SCORE_1 and DISPARITY_2 together (the pair replays exactly as the eager node runs it), not a fusing
 * DISPARITY_2 alone.  The frame must not overlap the node's buffers. */
int d2pc_fusion_node_callback_device(d2pc_fusion_node *node, int which, const void *d_frame, size_t pitch,
                                     size_t frame_stride, d2pc_fusion_node_topics *out, void *stream);

typedef struct d2pc_fusion_node_host_topics {
  uint32_t struct_size;               /* sizeof(d2pc_fusion_node_host_topics), set by the caller */
  uint32_t published;                 /* out: as above */
  void *data[D2PC_NODE_TOPICS];       /* in: HOST buffer per topic, rows packed (step = width x channels); NULL =
                                         do not copy that topic */
  size_t capacity[D2PC_NODE_TOPICS];  /* in: bytes each buffer holds */
  size_t bytes[D2PC_NODE_TOPICS];     /* out: bytes of each published topic (all pairs), copied unless data is NULL */
  int32_t width[D2PC_NODE_TOPICS], height[D2PC_NODE_TOPICS], channels[D2PC_NODE_TOPICS];  /* out */
} d2pc_fusion_node_host_topics;

/* The same for frames in HOST memory (mono8, `batch` frames packed pitch x rows apart), synchronous: upload, the
 * launches, download of the published topics.  A non-NULL buffer smaller than its topic gives D2PC_ERR_CAPACITY
 * BEFORE anything is enqueued: the node's state is as it was and the node stays usable. */
int d2pc_fusion_node_callback(d2pc_fusion_node *node, int which, const void *host_frame, size_t pitch,
                              d2pc_fusion_node_host_topics *io);

/*
 * A camera RIG as a session: n cameras of one geometry and sample type, each with its OWN Q, turned into ONE cloud by
 * one asynchronous call.  The reference is deployed on such a rig (hpp:71 "Omni-stereo"; its cloud topic is the merged
 * /omi_cam/point_cloud), and a batch of frames arises from n cameras at one instant, not from one camera n times.
 * A camera's pose is folded into its Q: [X Y Z W] = Q.(u,v,d,1), so a rigid T in front of Q is just another Q
 * (d2pc_rig_compose_q) and cv::reprojectImageTo3D's arithmetic stays the specification.
 *
 * Border, mode, min_disparity and the reproject form are the CONTEXT's, read at every d2pc_rig_process_device call:
 *   PARITY   camera f's (W-2b)(H-2b) points at point f * roi_points, reference order inside each camera
 *   COMPACT  the survivors of camera 0, then of camera 1, ...: dense, row-major inside each camera; the per-camera
 *            counts and start offsets are written on the device and the host never reads a count
 * The per-camera calibrations live in a table in device memory; a camera whose Q has cv::stereoRectify's structure
 * takes the specialised arithmetic, any other (a posed camera) the general one, exactly as d2pc_process_device
 * would with d2pc_set_q(that Q): same bytes.  D2PC_FORM_CV24 is refused (D2PC_ERR_INVALID_ARG): its per-row segments
 * are host work per Q and per width.
 */
#define D2PC_RIG_MAX_CAMERAS 64
typedef struct d2pc_rig_config {
  uint32_t struct_size;        /* sizeof(d2pc_rig_config) */
  int32_t n_cameras;           /* 1 .. D2PC_RIG_MAX_CAMERAS */
  int32_t width, height;       /* of every camera's frame */
  int32_t dtype;               /* D2PC_DTYPE_F32 / _U8 / _U16 */
  int32_t reserved[3];
} d2pc_rig_config;
/* struct_size, one camera, D2PC_DTYPE_F32; width = height = 0: the caller's to set. */
void d2pc_rig_config_init(d2pc_rig_config *cfg);

typedef struct d2pc_rig_geometry_t {
  size_t roi_points;           /* ROI points of one camera: d2pc_roi_points(width, height, border) */
  size_t capacity_points;      /* n_cameras * roi_points: what d_out_points (and d_out_index) must hold */
  size_t device_bytes;         /* device memory the session holds (calibration table + tile counts) */
  int32_t index_available;     /* 0 when n_cameras * width * height > 2^32: d_out_index is refused */
  int32_t reserved[3];
} d2pc_rig_geometry_t;
/* Host arithmetic only (no context, no device); the refusals are d2pc_rig_create's: D2PC_ERR_INVALID_ARG (NULL,
 * struct_size, n_cameras, border), D2PC_ERR_BAD_DTYPE, D2PC_ERR_BAD_SIZE (width or height <= 0, a frame beyond 2^31
 * pixels or a ROI beyond 2^28, n_cameras * roi_points >= 2^32).  A border wider than the frame gives 0 points. */
int d2pc_rig_geometry(const d2pc_rig_config *cfg, int border, d2pc_rig_geometry_t *out);

/* out = T.Q, row-major 4 x 4, host only: out[r][k] = ((t_r0*q_0k + t_r1*q_1k) + t_r2*q_2k) + t_r3*q_3k, every product
 * and sum rounded on its own (no fused multiply-add).  T need not be rigid; non-finite entries are refused
 * (D2PC_ERR_INVALID_ARG).  `out` may be `t` or `q`.  The identity leaves a stereoRectify Q with that structure. */
int d2pc_rig_compose_q(const double t[16], const double q[16], double out[16]);

typedef struct d2pc_rig d2pc_rig;
/* q: n_cameras x 16 doubles, camera after camera.  Allocates everything the session will ever need (sized for border
 * 0): d2pc_rig_process_device allocates nothing and can be captured into a graph in both modes without a warm-up.
 * The rig lives on `ctx`'s device and must be destroyed before the context. */
int d2pc_rig_create(d2pc_ctx *ctx, const d2pc_rig_config *cfg, const double *q, d2pc_rig **out);
/* Synchronous; the caller has no launch of this rig in flight.  A captured graph reads the table when it REPLAYS:
 * a replay after d2pc_rig_set_q uses the new Q. */
int d2pc_rig_set_q(d2pc_rig *rig, int camera, const double q[16]);
int d2pc_rig_get_q(const d2pc_rig *rig, int camera, double q_out[16]);
/*
 * The n resident frames (camera f at d_frames + f * frame_stride_bytes, rows row_stride_bytes apart; `scale` as in
 * d2pc_process_device) into one cloud at d_out_points (16-byte aligned), asynchronous on `stream` (NULL = the HIP
 * default stream).  capacity_points < n_cameras * roi_points gives D2PC_ERR_CAPACITY before anything is enqueued.
 * d_out_index (nullable) receives f * width * height + v * width + u, the pixel's index in the batch.
 * d_counts (n) and d_offsets (n + 1; d_offsets[n] = the cloud's points) are nullable in PARITY and required in
 * COMPACT.  The frames must not overlap the outputs.  The tile counts belong to the rig: one launch of a rig in
 * flight per stream order; two streams need two rigs.
 */
int d2pc_rig_process_device(d2pc_rig *rig, const void *d_frames, float scale, size_t row_stride_bytes,
                            size_t frame_stride_bytes, void *d_out_points, uint32_t *d_out_index,
                            size_t capacity_points, uint32_t *d_counts, uint32_t *d_offsets, void *stream);
int d2pc_rig_destroy(d2pc_rig *rig);

/*
 * TEXTURED clouds: pcl::PointXYZI / pcl::PointXYZRGB records (32 bytes) made from a cloud this library produced and a
 * per-pixel plane aligned with the disparity grid (the camera image; the fusion node's COMBINED_SCORE).  The texture
 * is attached BEHIND the producer by one memory-bound gather: every producer above already leaves each point's source
 * pixel (d_out_index) and the counts on the device, so one entry point serves every mode, every reproject form, the
 * callback body and the rig, and the first 16 bytes of a record are the producer's bytes by construction.
 *
 *   D2PC_POINT_XYZI    {x, y, z, 1.0f | intensity, 0, 0, 0}: intensity = (float)sample for the 8- and 16-bit texture
 *                      formats (exact), a bit copy of the sample for D2PC_TEX_F32 (NaN payloads included).  PCL leaves
 *                      the record's last 12 bytes indeterminate; here they are zero.
 *   D2PC_POINT_XYZRGB  {x, y, z, 1.0f | rgb, 0, 0, 0}: rgb is the 32-bit word (255 << 24) | (r << 16) | (g << 8) | b,
 *                      in memory the bytes b, g, r, 255.  Alpha 255 is what the constructors of PCL >= 1.8 set
 *                      (stereo_image_proc leaves 0): a documented choice, no release is pinned.  D2PC_TEX_RGB8 and
 *                      D2PC_TEX_BGR8 are packed 3-byte pixels (any pitch >= 3 W, no alignment); D2PC_TEX_MONO8 gives
 *                      r = g = b.
 * The point's 16 bytes are copied bit for bit (the pad 1.0f, a NaN coordinate).
 */
typedef enum d2pc_point_format { D2PC_POINT_XYZI = 1, D2PC_POINT_XYZRGB = 2 } d2pc_point_format;
typedef enum d2pc_texture_format {
  D2PC_TEX_U8 = 1,      /* XYZI   */
  D2PC_TEX_U16 = 2,     /* XYZI   */
  D2PC_TEX_F32 = 3,     /* XYZI   */
  D2PC_TEX_RGB8 = 4,    /* XYZRGB */
  D2PC_TEX_BGR8 = 5,    /* XYZRGB */
  D2PC_TEX_MONO8 = 6    /* XYZRGB */
} d2pc_texture_format;

typedef struct d2pc_texture_desc {
  uint32_t struct_size;        /* sizeof(d2pc_texture_desc) */
  int32_t point_format;        /* d2pc_point_format */
  int32_t texture_format;      /* d2pc_texture_format; must belong to the point format */
  int32_t width, height;       /* of the source frames the cloud was made from (and of the texture) */
  int32_t border;              /* the producer's border; read only when `index` is NULL */
  int32_t n_frames;            /* source frames = texture planes, 1 .. 65,535 */
  int32_t merged;              /* 0: n_frames clouds, cloud f from frame f, index v * width + u (what d2pc_process_device and
                                  d2pc_process_mono_device write); 1: ONE cloud, index f * width * height + v * width + u
                                  (what d2pc_rig_process_device writes) */
  const void *texture;         /* DEVICE: n_frames planes of height rows */
  size_t tex_pitch;            /* bytes between rows */
  size_t tex_frame_stride;     /* bytes between planes (ignored when n_frames == 1) */
  const void *points;          /* DEVICE: the producer's 16-byte records, 16-byte aligned */
  const uint32_t *index;       /* DEVICE, nullable: the producer's d_out_index.  NULL = the PARITY layout, merged 0 only:
                                  position i is ROI pixel (border + i / (width - 2 border), border + i % (width - 2 border))
                                  and cloud_points must equal d2pc_roi_points(width, height, border) */
  const uint32_t *counts;      /* DEVICE, nullable: points of each cloud (the producer's d_counts; for a rig pass
                                  d_offsets + n_cameras, the merged cloud's total).  NULL = cloud_points each.  A count
                                  above cloud_points is clamped; 0xFFFFFFFF (the in-band failure mark of
                                  d2pc_process_device) counts as 0 */
  size_t cloud_points;         /* records one cloud may hold, 1 .. 2^32 - 1 */
  size_t points_frame_stride_points;  /* points between the clouds in `points` and in `index` (ignored for one cloud) */
  void *out;                   /* DEVICE out: 32-byte records, 16-byte aligned */
  size_t out_frame_stride_points;     /* records between the clouds in `out` (ignored for one cloud) */
} d2pc_texture_desc;

/* struct_size, D2PC_POINT_XYZI, D2PC_TEX_U8, n_frames 1; everything else zero. */
void d2pc_texture_desc_init(d2pc_texture_desc *desc);
/*
 * Asynchronous on `stream` (NULL = the HIP default stream); allocates nothing, so it can be captured into a graph as
 * it is, behind its producer.  The context supplies the device and d2pc_last_error only: border and layout come from
 * the descriptor, so a cloud made earlier can be textured later.  Record i of a cloud is written for
 * i < min(cloud_points, count); records beyond stay untouched.  An index at or beyond the declared pixels (width x
 * height, merged: n_frames x width x height) gives texture word 0 and reads nothing.  No host round trip: the counts
 * are read on the device.
 * Refused before anything is enqueued: NULL or a wrong struct_size (D2PC_ERR_INVALID_ARG); an unknown format or a
 * texture format of the other point format (D2PC_ERR_BAD_DTYPE); width, height, n_frames <= 0, border < 0, width x
 * height > 2^31, merged n_frames x width x height > 2^32, cloud_points 0 or >= 2^32, a NULL index whose cloud_points is
 * not d2pc_roi_points, a texture plane that does not fit its pitch (< 2^32) or frame stride, a frame stride below
 * cloud_points or beyond 2^40 points, a tex_frame_stride beyond 2^46 bytes (D2PC_ERR_BAD_SIZE); a NULL index with merged 1, points / out not 16-byte aligned, a 16- or 32-bit
 * texture (base, pitch, frame stride), index or counts not aligned to their sample, `out` overlapping any input
 * (D2PC_ERR_INVALID_ARG).
 */
int d2pc_texture_device(d2pc_ctx *ctx, const d2pc_texture_desc *desc, void *stream);

/* sensor_msgs/PointCloud2 metadata of n textured records, as pcl::toROSMsg fills it for pcl::PointXYZI /
 * pcl::PointXYZRGB: point_step 32, row_step 32 n, fields x, y, z at 0 / 4 / 8 and "intensity" or "rgb" at 16, all
 * FLOAT32 (7), count 1.  ("intensity" does not fit d2pc_field's 8 bytes: a field type of its own.)  Host only, no
 * context.  D2PC_ERR_INVALID_ARG for NULL, D2PC_ERR_BAD_DTYPE for an unknown format, D2PC_ERR_BAD_SIZE when 32 n does
 * not fit 32 bits. */
typedef struct d2pc_textured_field { char name[12]; uint32_t offset; uint8_t datatype; uint32_t count; } d2pc_textured_field;
typedef struct d2pc_textured_cloud_meta {
  uint32_t height;        /* 1                                                */
  uint32_t width;         /* n                                                */
  uint32_t point_step;    /* 32 = sizeof(pcl::PointXYZI / pcl::PointXYZRGB)   */
  uint32_t row_step;      /* 32*n                                             */
  uint8_t is_bigendian;   /* 0                                                */
  uint8_t is_dense;       /* as given                                         */
  uint32_t n_fields;      /* 4                                                */
  d2pc_textured_field fields[4];
} d2pc_textured_cloud_meta;
int d2pc_textured_cloud_meta_fill(int point_format, size_t n_points, int is_dense, d2pc_textured_cloud_meta *meta);

#ifdef __cplusplus
}
#endif
#endif /* D2PC_H */
