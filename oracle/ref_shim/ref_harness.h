/* ref_harness.h -- the C ABI of oracle/_ref/libref_fusion.so: the reference's DepthMapFusion, compiled unmodified
 * against the stand-in headers of this directory.  See ref_harness.cpp and oracle/ref.py. */
#ifndef D2PC_REF_HARNESS_H
#define D2PC_REF_HARNESS_H
#include <stddef.h>
#include <stdint.h>

#include "opencv2/imgproc/imgproc.hpp" /* ref_view and the three hook types */

#ifdef __cplusplus
extern "C" {
#endif

enum { REF_OK = 0, REF_THREW = 1, REF_NO_HOOK = 2, REF_BAD_ARG = 3 };
enum { REF_DISPARITY_1 = 0, REF_DISPARITY_2 = 1, REF_MATCHING_SCORE_1 = 2, REF_MATCHING_SCORE_2 = 3 };

typedef struct ref_node ref_node;

typedef struct ref_topic {
  const char *topic, *encoding, *frame_id;
  uint32_t seq, width, height, step;
  const uint8_t *data;
  size_t bytes;
} ref_topic;

const char *ref_last_error(void);
void ref_set_hooks(ref_gaussian_hook gaussian, ref_sobel_hook sobel, ref_threshold_hook threshold);

/* rule 0..8 in the order of the reference's source (weightedAverage .. gradFilter); g1 / g2 may be null (0).
 * out[i] = -1 where rule 0 would divide by zero (both scores non-zero: both int weights are 0). */
int ref_fuse_pixels(int rule, size_t count, const uint8_t *d1, const uint8_t *d2, const uint8_t *s1, const uint8_t *s2,
                    const uint8_t *g1, const uint8_t *g2, int16_t *out);

/* rect = x, y, width, height of the returned view inside the image; REF_THREW is an outcome */
int ref_crop_to_square(int cols, int rows, int offset_x, int offset_y, int member_offset_y, int rect[4]);
int ref_crop_mat(int cols, int rows, int left, int right, int top, int bottom, int rect[4]);
int ref_rotate_mat(const uint8_t *src, size_t step, int cols, int rows, uint8_t *dst, int dst_size[2]);
int ref_colorize(const uint8_t *gray, size_t step, int cols, int rows, int as_view, uint8_t *rgb);
/* returns a bit per stage of the reference that threw (ref_harness.cpp); 0 = none */
int ref_geometry(int cols, int rows, int offset_x, int offset_y, int out[16]);
int ref_geometry_batch(size_t count, const int *cols, const int *rows, const int *offset_x, const int *offset_y, int *out,
                       int *status);

ref_node *ref_node_create(int offset_x, int offset_y, int have_offset_x, int have_offset_y);
void ref_node_destroy(ref_node *node);
int ref_node_warnings(void);
int ref_node_offsets(const ref_node *node, int out[2]);
/* runs one callback on a mono8 frame; afterwards ref_node_published / ref_node_topic list what it published, in order */
int ref_node_callback(ref_node *node, int which, const uint8_t *frame, size_t step, int cols, int rows, uint32_t seq,
                      const char *frame_id);
int ref_node_published(const ref_node *node);
int ref_node_topic(const ref_node *node, int index, ref_topic *out);

#ifdef __cplusplus
}
#endif
#endif
