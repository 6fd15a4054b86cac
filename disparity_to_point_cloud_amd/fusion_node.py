"""The depth_map_fusion node (reference src/depth_map_fusion.cpp) as a device-resident session: the four callbacks,
the state they share and the seven topics they publish.  torch owns the memory and the streams; every byte is
computed by libd2pc.so's HIP kernels (d2pc_colorize_device, d2pc_score_filter_device, d2pc_rotate_cw_device,
d2pc_fuse_device).

Reference launch parameters (launch/depth_map_fusion.launch): 752 x 480 frames, offset_x -7, offset_y 15, which
give n = 465 and a 425 x 425 fused map:

    node = FusionNode(ctx, 752, 480, offset_x=-7, offset_y=15)
    node.matching_score_1(score1); node.matching_score_2(score2); node.disparity_1(disp1)
    topics = node.disparity_2(disp2)      # cropped_depth_2, combined_score, gradient, fused_depth_map
"""
import torch

from . import capi

CROP = (0, 40, 30, 10)  # cropMat(.., 0, 40, 30, 10) of publishFusedDepthMap (:130): left, right, top, bottom


class FusionNode:
    """State and callbacks of DepthMapFusion for `batch` independent camera pairs.

    Everything is allocated here, so every callback is a fixed sequence of kernel launches on torch's current
    stream -- disparity_1: 1, disparity_2: 3 (1 before all four planes have arrived), matching_score_1: 1,
    matching_score_2: 2 -- with no allocation and no device-to-device copy, and can be captured by torch.cuda.graph.

    Frames are uint8 CUDA tensors of shape (rows, cols), or (batch, rows, cols) when batch > 1, with unit column
    stride; anything else raises ValueError (mono16: convert with Context.mono16_to_mono8_device first).  The
    callbacks return {topic: tensor}.  The tensors are the session's own buffers: a topic's tensor is overwritten by
    the next callback that publishes that topic, and `combined_score` and `cropped_score_1` additionally by the next
    matching_score_1 / disparity_2, because the reference keeps camera 1's score, its grad and the combined
    confidence in ONE buffer (:77,:113): each fusion leaves min(grad1, grad2) in camera 1's score plane until the next
    matching_score_1, and a disparity_2 without new scores fuses against that.  The session reproduces this by
    swapping two buffers, never by copying.  Which buffer is which is host state: a captured callback is pinned to
    the planes it was captured with, so capture matching_score_1 and disparity_2 together (the pair replays exactly
    as the eager node runs it) rather than a fusing disparity_2 alone."""

    def __init__(self, ctx: capi.Context, cols, rows, offset_x=0, offset_y=0, rule=capi.FUSE_GRAD_FILTER,
                 form=capi.SCORE_FORM_CV4, batch=1, device="cuda:0"):
        if batch < 1:
            raise ValueError("batch must be >= 1")
        self.ctx, self.cols, self.rows, self.batch = ctx, int(cols), int(rows), int(batch)
        self.rule, self.form = rule, form
        self.device = torch.device(device)
        # publishFusedDepthMap re-crops its frame with the side min(cols, rows) - |offset_y| (:106, :253) and fuses only
        # min(cols, rows) - max(|offset_x|, |offset_y|) of it: with |offset_x| > |offset_y| the reference publishes a
        # larger fused map with a margin of raw camera-2 pixels.  Refused, as d2pc_fusion_node_geometry refuses it
        # (D2PC_ERR_BAD_SIZE)
        if abs(offset_x) > abs(offset_y):
            raise capi.D2pcError(3, "fusion node %dx%d: |offset_x| (%d) exceeds |offset_y| (%d): not supported"
                                 % (self.cols, self.rows, offset_x, offset_y))
        # camera 1: cropToSquare(image, offset_x, offset_y); camera 2: of the ROTATED image (rows x cols) with the
        # negated offsets -- while the side length still uses the member offset_y_ (:253)
        self.sq1 = capi.crop_to_square(self.cols, self.rows, offset_x, offset_y)
        self.sq2 = capi.crop_to_square(self.rows, self.cols, -offset_x, -offset_y, offset_y)
        if self.sq1[2] != self.sq2[2]:
            raise ValueError("the two cameras' squares differ in size")
        n = self.n = self.sq1[2]
        l, r, t, b = CROP
        self.fused_w, self.fused_h = n - l - r, n - t - b
        if n < 11 or self.fused_w < 1 or self.fused_h < 1:
            raise ValueError("square of %d pixels: too small for the score filter and the crop" % n)
        u8 = dict(dtype=torch.uint8, device=self.device)
        B = self.batch
        self._rot = torch.empty((B, self.cols, self.rows), **u8)   # camera 2's score frame, rotated
        self._depth = [torch.empty((B, n, n), **u8) for _ in range(2)]
        self._score1, self._spare = torch.empty((B, n, n), **u8), torch.empty((B, n, n), **u8)
        self._score2 = torch.empty((B, n, n), **u8)
        self._color = [torch.empty((B, n, n, 3), **u8) for _ in range(2)]
        self._fused = torch.empty((B, self.fused_h, self.fused_w), **u8)
        self._gradient = torch.empty((B, self.fused_h, self.fused_w, 3), **u8)
        self._have = {"depth_1": False, "depth_2": False, "score_1": False, "score_2": False}

    # -- helpers -------------------------------------------------------------------------------------------------
    def _frame(self, frame):
        return capi.device_frames(frame, self.rows, self.cols, self.batch)

    def _out(self, t):
        return t[0] if self.batch == 1 else t

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _colorize(self, src, cols, rows, pitch, fstride, rotate, view, gray, rgb):
        d = capi.colorize_desc_init()
        d.rotate_cw, d.cols, d.rows, d.n_frames = rotate, cols, rows, self.batch
        d.x, d.y, d.w, d.h = view
        d.src, d.src_pitch, d.src_frame_stride = src.data_ptr(), pitch, fstride
        if gray is not None:
            d.gray, d.gray_pitch, d.gray_frame_stride = gray.data_ptr(), gray.stride(1), gray.stride(0)
        d.rgb, d.rgb_pitch, d.rgb_frame_stride = rgb.data_ptr(), rgb.stride(1), rgb.stride(0)
        self.ctx.colorize_device(d, self._stream())

    def _score_filter(self, src, width, height, pitch, fstride, sq, direction, out):
        d = capi.score_filter_desc_init()
        d.direction, d.form, d.width, d.height, d.n_frames = direction, self.form, width, height, self.batch
        d.x, d.y, d.n = sq
        d.src, d.src_pitch, d.src_frame_stride = src.data_ptr(), pitch, fstride
        d.out, d.out_pitch, d.out_frame_stride = out.data_ptr(), out.stride(1), out.stride(0)
        self.ctx.score_filter_device(d, self._stream())

    def _strides(self, frame):
        return frame.stride(-2), (frame.stride(0) if frame.dim() == 3 else 0)

    # -- the callbacks -------------------------------------------------------------------------------------------
    def disparity_1(self, frame):
        """DisparityCb1 (:45-51): one launch.  -> {cropped_depth_1: n x n x 3}"""
        frame = self._frame(frame)
        pitch, fstride = self._strides(frame)
        x, y, n = self.sq1
        self._colorize(frame, self.cols, self.rows, pitch, fstride, 0, (x, y, n, n), self._depth[0], self._color[0])
        self._have["depth_1"] = True
        return {"cropped_depth_1": self._out(self._color[0])}

    def disparity_2(self, frame):
        """DisparityCb2 (:53-61): the rotated view and its colouring (one launch), then -- once all four planes
        have arrived (:106-109) -- publishFusedDepthMap: fuse + median + crop (one launch) and the colouring of the
        fused map (one launch).  -> {cropped_depth_2[, combined_score, gradient, fused_depth_map]}.
        `combined_score` stays valid until the next matching_score_1 or disparity_2."""
        frame = self._frame(frame)
        pitch, fstride = self._strides(frame)
        x, y, n = self.sq2
        self._colorize(frame, self.cols, self.rows, pitch, fstride, 1, (x, y, n, n), self._depth[1], self._color[1])
        self._have["depth_2"] = True
        out = {"cropped_depth_2": self._out(self._color[1])}
        if not all(self._have.values()):
            return out
        s1, s2, comb = self._score1, self._score2, self._spare
        d = capi.fuse_desc_init()
        d.rule, d.width, d.height, d.n_frames = self.rule, n, n, self.batch
        d.crop_left, d.crop_right, d.crop_top, d.crop_bottom = CROP
        for i, p in enumerate((self._depth[0], self._depth[1], s1, s2, s1, s2)):  # score and grad: one plane (:77,:96)
            d.planes[i], d.pitch[i], d.frame_stride[i] = p.data_ptr(), p.stride(1), p.stride(0)
        d.fused, d.fused_pitch, d.fused_frame_stride = self._fused.data_ptr(), self._fused.stride(1), self._fused.stride(0)
        d.combined, d.combined_pitch, d.combined_frame_stride = comb.data_ptr(), comb.stride(1), comb.stride(0)
        self.ctx.fuse_device(d, self._stream())
        # cropped_score_combined_ IS cropped_score_1_ (:113): from now on camera 1's score/grad plane is the combined one
        self._score1, self._spare = comb, s1
        self._colorize(self._fused, self.fused_w, self.fused_h, self._fused.stride(1), self._fused.stride(0), 0,
                       (0, 0, self.fused_w, self.fused_h), None, self._gradient)
        out["combined_score"] = self._out(self._score1)
        out["gradient"] = self._out(self._gradient)
        out["fused_depth_map"] = self._out(self._fused)
        return out

    def matching_score_1(self, frame):
        """MatchingScoreCb1 (:64-80): one launch.  -> {cropped_score_1: n x n, the filtered score}"""
        frame = self._frame(frame)
        pitch, fstride = self._strides(frame)
        self._score_filter(frame, self.cols, self.rows, pitch, fstride, self.sq1, 0, self._score1)
        self._have["score_1"] = True
        return {"cropped_score_1": self._out(self._score1)}

    def matching_score_2(self, frame):
        """MatchingScoreCb2 (:82-99): rotate, filter (two launches; the filter's first blur reads the rotated
        frame's pixels round the square).  -> {cropped_score_2: n x n}"""
        frame = self._frame(frame)
        pitch, fstride = self._strides(frame)
        rot = self._rot
        self.ctx.rotate_cw_device(frame.data_ptr(), self.cols, self.rows, pitch, fstride, self.batch, rot.data_ptr(),
                                  rot.stride(1), rot.stride(0), self._stream())
        self._score_filter(rot, self.rows, self.cols, rot.stride(1), rot.stride(0), self.sq2, 1, self._score2)
        self._have["score_2"] = True
        return {"cropped_score_2": self._out(self._score2)}
