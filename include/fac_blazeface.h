/* fac_blazeface.h - C ABI of the gfx950 BlazeFace face detector.
 *
 * Replaces `helpers/blazeface.py` (the MediaPipe BlazeFace front model: 128x128
 * input, 896 anchors) and the tile / untile / NMS / margin flow around it
 * (`helpers/helpers_face_extract_1.py:76-131,139-299`).  Everything is fp32.
 *
 * Conventions are those of fac_cvit.h: every function returns FAC_OK (0) or a
 * negative fac_status, nothing is thrown; d_* pointers are device pointers
 * owned by the caller; `stream` is a hipStream_t (NULL = default stream) and
 * all work is stream-ordered.  The handle owns the packed weights, the anchors
 * and a workspace; the workspace is allocated at the first call at a given
 * tile / frame count and reused afterwards (no allocation in later calls).
 *
 * Frames are uint8 [F, H, W, 3] as decoded (no channel swap).  A frame is cut
 * into n windows of side split = min(H, W) at y = 0, (W - split) / 2 apart:
 * n = 3 if W > H, else 1; each window is area-averaged to a 128x128 tile
 * (exact integer arithmetic, round half up).  min(H, W) < 128 is
 * FAC_ERR_SHAPE: there is no upscale path.
 *
 * A detection is 17 floats: ymin, xmin, ymax, xmax, six keypoints (x, y),
 * score.  Tile detections are normalised to the tile; frame detections are in
 * frame pixels.  A box is 5 int32: frame, left, top, right, bottom (what
 * fac_crop_resize_u8 takes).
 */
#ifndef FAC_BLAZEFACE_H
#define FAC_BLAZEFACE_H

#include "fac_cvit.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fac_bf fac_bf;

/* Candidates the per-frame NMS keeps (1024): the size of the second dimension
 * of every per-frame output below. */
int fac_bf_capacity(void);

int fac_bf_create(int device, fac_bf** out);
void fac_bf_destroy(fac_bf* h);

/* The 74 tensors of the reference state_dict (backbone1.0.weight ...
 * regressor_16.bias) plus "anchors" [896, 4], as host fp32 tensors by name.
 * Packs and uploads; synchronous. */
int fac_bf_load(fac_bf* h, const fac_tensor_desc* descs, int n);

/* frames -> tiles -> net -> decode -> per-frame untile, weighted NMS, margin.
 *   d_dets     [F, capacity, 17]  frame detections before the margin
 *   d_boxes    [F, capacity, 5]   margin boxes, truncated toward zero
 *   d_counts   [F]                valid rows of the two above
 *   d_overflow [F]                candidates beyond `capacity` that were
 *                                 dropped (the lowest scoring ones) */
int fac_bf_detect(fac_bf* h, const uint8_t* d_frames, int F, int H, int W, float min_score, float min_iou,
                  float* d_dets, int32_t* d_boxes, int32_t* d_counts, int32_t* d_overflow, void* stream);

/* 128x128 tiles uint8 [T, 128, 128, 3] -> per-tile detections in anchor order:
 * d_dets [T, 896, 17], d_counts [T] (predict_on_batch(apply_nms=False)). */
int fac_bf_tile_detections(fac_bf* h, const uint8_t* d_tiles, int T, float min_score, float* d_dets,
                           int32_t* d_counts, void* stream);

/* Weighted NMS of G independent lists, d_dets [G, stride, 17] with d_counts[g]
 * valid rows each (stride <= 2688), coordinates left as they are:
 * d_out [G, capacity, 17], d_out_counts [G], d_overflow [G]. */
int fac_bf_nms(fac_bf* h, const float* d_dets, const int32_t* d_counts, int G, int stride, float min_iou,
               float* d_out, int32_t* d_out_counts, int32_t* d_overflow, void* stream);

/* Debug: the tiles of fac_bf_detect, d_tiles uint8 [F * n, 128, 128, 3]. */
int fac_bf_debug_tiles(fac_bf* h, const uint8_t* d_frames, int F, int H, int W, uint8_t* d_tiles, void* stream);

/* Debug: the net on tiles; any output may be NULL.  NHWC fp32:
 * d_b1 [T, 16, 16, 88] (backbone1), d_b2 [T, 8, 8, 96] (backbone2),
 * d_r [T, 896, 16], d_c [T, 896, 1] (the raw tensors, anchor order). */
int fac_bf_debug_net(fac_bf* h, const uint8_t* d_tiles, int T, float* d_b1, float* d_b2, float* d_r, float* d_c,
                     void* stream);

/* Debug: one layer kernel of the net, one launch, on caller-owned buffers with
 * the loaded weights (no workspace).  NHWC fp32.
 *   stem   d_tiles uint8 [T, 128, 128, 3] -> d_out [T, 64, 64, 24]
 *   block  BlazeBlock `index` 0..15 (backbone1.2 .. backbone1.12, then
 *          backbone2.0 .. backbone2.4): d_in [T, hin, hin, cin] ->
 *          d_out [T, hin / stride, hin / stride, cout]
 *   heads  d_b1 [T, 16, 16, 88], d_b2 [T, 8, 8, 96] -> d_r [T, 896, 16],
 *          d_c [T, 896]
 * An index outside 0..15 is FAC_ERR_ARG. */
int fac_bf_debug_stem(fac_bf* h, const uint8_t* d_tiles, int T, float* d_out, void* stream);
int fac_bf_debug_block(fac_bf* h, int index, const float* d_in, int T, float* d_out, void* stream);
int fac_bf_debug_heads(fac_bf* h, const float* d_b1, const float* d_b2, int T, float* d_r, float* d_c,
                       void* stream);

/* Debug: the post-processing of fac_bf_detect from caller-supplied raw
 * tensors of F * n tiles.  d_tile_dets [F * n, 896, 17] and d_tile_counts
 * [F * n] may be NULL; the rest as fac_bf_detect. */
int fac_bf_debug_postprocess(fac_bf* h, const float* d_r, const float* d_c, int F, int H, int W, float min_score,
                             float min_iou, float* d_tile_dets, int32_t* d_tile_counts, float* d_dets,
                             int32_t* d_boxes, int32_t* d_counts, int32_t* d_overflow, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FAC_BLAZEFACE_H */
