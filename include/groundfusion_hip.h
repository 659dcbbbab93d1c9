/* groundfusion_hip.h — C-ABI of the MI355X-native Ground-Fusion hot path (libgroundfusion_hip.so).
 *
 * Drop-in boundary.  The reference has no FFI layer: the boundary is the C++ class surface
 *   FeatureTracker::trackImage      vins_estimator/src/featureTracker/feature_tracker.h:47
 *   FeatureTracker::setPrediction   feature_tracker.h:70
 *   FeatureTracker::removeOutliers  feature_tracker.h:72
 *   Estimator::optimization         vins_estimator/src/estimator/estimator.h (called from processImage, estimator.cpp:1112)
 * Each entry point below names the reference interface it replaces.  Plain pointers and sizes only; no
 * exceptions cross this boundary; every function returns GF_OK (0) or a negative gf_status and records a
 * message retrievable with gf_last_error().  One handle drives `batch` independent sequences on one GPU
 * (batch = 1 reproduces the reference's one-FeatureTracker-per-process use); handles are not re-entrant
 * (same rule as the reference objects, estimator.cpp:209-239).
 */
#ifndef GROUNDFUSION_HIP_H
#define GROUNDFUSION_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gf_status {
    GF_OK = 0,
    GF_ERR_INVALID = -1,   /* bad argument */
    GF_ERR_NO_DEVICE = -2, /* no HIP device / HIP runtime failure: the product path never falls back to CPU */
    GF_ERR_HIP = -3,
    GF_ERR_CAPACITY = -4   /* caller buffer too small */
} gf_status;

const char* gf_last_error(void);
int gf_device_count(int* n);
int gf_set_device(int device);

/* ------------------------------------------------------------------ front end: FeatureTracker */
typedef struct gf_tracker gf_tracker;

/* Pixel formats of the frames a tracker handle is given and of gf_cvt_gray_batch*: what getImageFromMsg (rosNodeTest.cpp:238-254) accepts before
 * cv_bridge::toCvCopy(msg, MONO8) -- mono8 / 8UC1, rgb8, bgr8, rgba8, bgra8 -- with 1, 3, 3, 4, 4 bytes per pixel, and the raw formats of cameras that do not
 * debayer on board: bayer_rggb8 / _bggr8 / _gbrg8 / _grbg8 (1 byte per pixel; the four letters are the colours of pixels (0,0), (0,1), (1,0), (1,1); at least
 * 3 x 3), yuv422 (UYVY) and yuv422_yuy2 (2 bytes per pixel), mono16 of an image topic (2 bytes per pixel, little-endian).  5, 6 and 7 are no formats. */
enum { GF_PIX_MONO8 = 0, GF_PIX_RGB8, GF_PIX_BGR8, GF_PIX_RGBA8, GF_PIX_BGRA8,
       GF_PIX_BAYER_RGGB8 = 8, GF_PIX_BAYER_BGGR8, GF_PIX_BAYER_GBRG8, GF_PIX_BAYER_GRBG8, GF_PIX_YUV422_UYVY, GF_PIX_YUV422_YUY2, GF_PIX_MONO16 };

typedef struct gf_tracker_cfg {
    int width, height;  /* ROW/COL, parameters.cpp:138ff (image_height/image_width) */
    int batch;          /* number of independent sequences driven by this handle (>=1) */
    int max_cnt;        /* MAX_CNT   config/realsense/m2dgrp.yaml:131 */
    int min_dist;       /* MIN_DIST  m2dgrp.yaml:132 */
    int flow_back;      /* FLOW_BACK m2dgrp.yaml:136 */
    int depth_cam;      /* FeatureTracker::depth_cam, feature_tracker.h:95 */
    double fx, fy, cx, cy, k1, k2, p1, p2; /* camodocal pinhole, config/realsense/wt_cam.yaml */
    /* EQUALIZE (m2dgrp.yaml `equalize`, rosNodeTest.cpp:256-261): 1 = cv::createCLAHE() with its defaults (clip limit 40, 8 x 8 tiles) applied to every gray
     * frame on the device before the pyramid, into a buffer of the handle (the caller's frames, device ones included, are never modified; depth images are
     * not touched); 0 = off (the reference's FeatureTracker itself never equalises: its node does) */
    int equalize;
    /* The format of every frame the handle is given (GF_PIX_*; rosNodeTest.cpp:238-254, the cv_bridge::toCvCopy(msg, MONO8) of getImageFromMsg).  0 = GF_PIX_MONO8:
     * the handle as it always was -- no further buffer, no further launch.  A colour format: every entry point that takes frames (gf_tracker_track, _track_batch,
     * _track_some, _prefetch_batch, _prefetch_some / _track_prefetched, _track_batch_device, _track_some_device) reads them in that format and the handle converts
     * them to MONO8 on the device, into a buffer of its own, ahead of the equalisation and the pyramid: (R 4899 + G 9617 + B 1868 + 2^13) >> 14, alpha ignored,
     * the bits of OpenCV 4.2's cvtColor.  A raw format (GF_PIX_BAYER_*, GF_PIX_YUV422_*, GF_PIX_MONO16) is converted at the same place: Bayer by the bilinear
     * demosaic fused with that luma sum (cvtColor(COLOR_Bayer??2GRAY), generic loop), YUV 4:2:2 by taking the luma bytes, MONO16 by (v + 128) / 257 on
     * little-endian pixels.  The caller's frames are never written.  Host entry points: `stride` is bytes per row and must be >= width x bytes per pixel;
     * the staged path copies the frame as it is under the previous frame's kernels and converts on the tracking stream once the copy has landed.  Device entry
     * points: the frames are tight height x width x bytes per pixel, back to back in list order, or -- the _refs forms -- one pointer and row pitch per listed
     * sequence (gf_frame_ref).  This is the format of every sequence that has none of its own: a fleet of cameras with mixed
     * encodings sets them per sequence (gf_tracker_set_seq_format).  Anything outside GF_PIX_MONO8 .. GF_PIX_BGRA8 and GF_PIX_BAYER_RGGB8 .. GF_PIX_MONO16 is refused by gf_tracker_create. */
    int pixel_format;
} gf_tracker_cfg;

/* One element of trackImage's return value map<int, vector<pair<int, Matrix<double,8,1>>>>
 * (feature_tracker.cpp:344-368): v = (x_n, y_n, 1, u, v, vx, vy, depth_m). */
typedef struct gf_feature_obs {
    int id;
    int camera_id;
    double v[8];
} gf_feature_obs;

typedef struct gf_tracker_stats {
    /* accumulated since the last gf_tracker_reset_stats(); times from hipEvents on the handle's stream */
    double ms_pyramid, ms_lk, ms_detect, ms_total_gpu;
    /* host wall-clock split of the same frames: enqueue/pack, wait for LK, setMask bookkeeping, wait for detector, pack output */
    double ms_host_pre, ms_wait_lk, ms_host_mid, ms_wait_detect, ms_host_post;
    long long frames;            /* calls that processed at least one sequence */
    long long lk_launches;       /* launches of the LK kernel */
    long long lk_points;         /* points submitted to LK */
    long long lk_level_passes;   /* sum over points of pyramid levels actually processed (fwd+reverse) */
    long long lk_iterations;     /* sum over points/levels of Gauss-Newton iterations */
    long long tracked_features;  /* features that survived tracking (status==1 after all checks) */
    long long output_features;   /* features returned to the caller (tracked + newly detected) */
    /* branches of the corner selection, counted on the host from each sequence's candidate count and want:
     * select_streamed: sequences served by select_topk_kernel (want <= 16) with more than 4 096 candidates (the list past the registers is streamed every round);
     * select_global_sort: sequences that select_corners_kernel sorted in global memory (candidates beyond the handle's LDS sort area, 16 384 keys or fewer
     * when min_dist is small) */
    long long select_streamed;
    long long select_global_sort;
    double ms_equalize;          /* the CLAHE kernels of gf_tracker_cfg.equalize (hipEvents, like ms_pyramid; part of ms_total_gpu) */
    /* launches of each pyramid form, counted on the host where the pyramid is launched (the form follows the frame size, the pointers' alignment and GF_PYR_HEAD):
     * pyr_head: levels 0 + 1 in one kernel; pyr_level0_vec16 / pyr_level0_dword: level 0 alone in 16- / 4-byte pieces; pyr_down_tail: levels 2 .. 3 in one kernel;
     * pyr_down_pad4: one level >= 1 in four-pixel pieces; pyr_down_bytes: one level >= 1 one byte per thread */
    long long pyr_head, pyr_level0_vec16, pyr_level0_dword, pyr_down_tail, pyr_down_pad4, pyr_down_bytes;
    /* frames handed over by reference (gf_frame_ref) that missed the widest load form of the first kernel that read them, summed over the listed sequences of
     * the _refs calls: pointer or pitch no multiple of 16 where the pyramid or CLAHE reads the caller's frame, no multiple of 4 where a conversion kernel does;
     * 0 on a handle that only uses the other entry points */
    long long frames_unaligned;
    double ms_convert;           /* the colour / raw -> MONO8 kernels of pixel_format (hipEvents, like ms_equalize; part of ms_total_gpu); grows on the calls that convert a listed sequence */
    long long sequence_frames;   /* listed sequences summed over the calls (`frames` counts the calls): frames x batch for the lock-step entry points; stays the last member */
} gf_tracker_stats;

int gf_tracker_create(const gf_tracker_cfg* cfg, gf_tracker** out);
int gf_tracker_destroy(gf_tracker* h);

/* Replaces FeatureTracker::trackImage(t, img, depth) for sequence `seq` (feature_tracker.h:47) of a handle of any batch: the other sequences keep their state.
 * gray: height x width u8 (stride bytes); depth: height x width u16 millimetres (dstride elements) or NULL.
 * out/cap: caller-owned; *n_out = number of observations written (order = the tracker's `ids` vector). */
int gf_tracker_track(gf_tracker* h, int seq, double t, const uint8_t* gray, int stride, const uint16_t* depth,
                     int dstride, gf_feature_obs* out, int cap, int* n_out);

/* Same for all `batch` sequences in one pass; gray[b]/depth[b] are host images, out is [batch][cap].
 * On the host-image entry points (gf_tracker_track, _track_batch, _prefetch_batch / _track_prefetched) the depth image never crosses the bus: the reference reads one
 * pixel of it per feature (feature_tracker.cpp:360 `rightImg.at<ushort>(round(y), round(x))`), and those <= max_cnt samples are taken on the host from the caller's
 * image behind the kernels (round 5: a VGA RGB-D frame costs 307 KB of PCIe traffic instead of 921 KB). */
int gf_tracker_track_batch(gf_tracker* h, const double* t, const uint8_t* const* gray, int stride,
                           const uint16_t* const* depth, int dstride, gf_feature_obs* out, int cap, int* n_out);

/* The same boundary without serialising on the bus: gf_tracker_prefetch_batch starts the host -> device copy of the NEXT frame (a second pair of frame buffers,
 * a copy stream) and returns; gf_tracker_track_prefetched runs trackImage on the OLDEST staged frame as soon as its copy has landed.  Up to two frames can
 * be staged; call order: prefetch(0), then per frame k: prefetch(k + 1), track_prefetched(k) -- the copy of k + 1 runs under the kernels of k.  The host images -- the depth images in particular, which are sampled by track_prefetched itself -- must stay valid until the matching track_prefetched returns; only page-locked memory (gf_host_alloc,
 * or the caller's hipHostRegister) makes the copy overlap.  Images that lie back to back in one allocation travel as one copy per plane. */
/* One caller thread per tracker handle: prefetch / track_prefetched keep an unsynchronised two-slot FIFO, like every other gf_tracker_* entry point they must not
 * be called concurrently on the same handle. */
int gf_tracker_prefetch_batch(gf_tracker* h, const uint8_t* const* gray, int stride, const uint16_t* const* depth, int dstride);
int gf_tracker_track_prefetched(gf_tracker* h, const double* t, gf_feature_obs* out, int cap, int* n_out);
int gf_host_alloc(size_t bytes, void** out);
int gf_host_free(void* p);

/* Same with the images already resident in HBM: d_gray = batch contiguous height*width u8 images,
 * d_depth = batch contiguous height*width u16 images (or NULL).  Device pointers of the current device. */
int gf_tracker_track_batch_device(gf_tracker* h, const double* t, const void* d_gray, const void* d_depth,
                                  gf_feature_obs* out, int cap, int* n_out);

/* The sequences of a handle advance independently: a call names the `count` sequences that have a frame (seq[count], distinct, any order), and only those run
 * FeatureTracker::trackImage (feature_tracker.h:47).  A sequence that is not listed keeps its whole state -- tracks, ids, track_cnt, prev_time, its previous
 * pyramid, a pending prediction -- as if the call had not happened, so cameras that drop frames, start late, stop early or tick at different rates share one
 * handle.  Everything of the call is indexed by the position in the list: t[i], gray[i], depth[i], out[i * cap ..] and n_out[i] belong to sequence seq[i]
 * (the layout gf_estimator_group_submit_features reads with the same list), and the kernels, copies and host work of the call follow `count`, not the batch.
 * gf_tracker_track_batch* are these calls with the list 0 .. batch-1.  A refused call (GF_ERR_INVALID: count < 0 or > batch, an entry out of range, a sequence
 * named twice, a null image) changes nothing; count == 0 succeeds and does nothing. */
/* trackImage (feature_tracker.h:47) on host images of the listed sequences; depth as in gf_tracker_track_batch (NULL, or one image per listed sequence) */
int gf_tracker_track_some(gf_tracker* h, int count, const int* seq, const double* t, const uint8_t* const* gray, int stride,
                          const uint16_t* const* depth, int dstride, gf_feature_obs* out, int cap, int* n_out);
/* trackImage (feature_tracker.h:47) on device images: d_gray / d_depth hold the `count` frames of the listed sequences back to back, in list order */
int gf_tracker_track_some_device(gf_tracker* h, int count, const int* seq, const double* t, const void* d_gray, const void* d_depth,
                                 gf_feature_obs* out, int cap, int* n_out);
/* A frame that already lives on the device, where its producer keeps it: the device pointer (current device) of the first byte of row 0 and the bytes from one
 * row to the next.  Any byte alignment of both; pitch >= width x bytes per pixel of the sequence's pixel format (the handle's, or its own: gf_tracker_set_seq_format).  Frames of one call may lie in different
 * allocations, be views into larger surfaces (the luma plane of an NV12 / I420 surface, a crop of a wider image) and may alias each other.  Nothing behind a
 * gf_frame_ref is ever written. */
typedef struct gf_frame_ref { const void* data; size_t pitch; } gf_frame_ref;
/* trackImage (feature_tracker.h:47) on device images that are handed over by reference: gray[i] is the frame of seq[i] in that sequence's pixel format (height rows
 * of width x bytes per pixel), depth is NULL or one entry per listed sequence of u16 millimetres (data and pitch even; an entry with data == NULL is allowed
 * exactly for a sequence whose depth_cam is 0).  Every other property of the call -- list semantics, count == 0, sequences that sit out, setPrediction /
 * removeOutliers, parameters per sequence, region of interest, equalize, statistics, synchronisation -- is that of gf_tracker_track_some_device, which is the
 * case "frame i at base + i x frame bytes, pitch = row bytes" of the same path and gives the same bits for the same pixels.  Only the first kernel that reads the
 * caller's memory addresses it through the table (16-byte pieces for a frame whose pointer and pitch are multiples of 16, dwords or bytes otherwise; one call may
 * mix them; gf_tracker_stats.frames_unaligned counts the others); the handle's first such call allocates the table.  Refused with GF_ERR_INVALID, the message
 * naming the list position, and nothing changed: a null table, a null data pointer where one is needed, a pitch shorter than a row, an odd depth pointer or
 * pitch, and everything gf_tracker_track_some_device refuses.  The pointers are not validated beyond that. */
int gf_tracker_track_some_device_refs(gf_tracker* h, int count, const int* seq, const double* t, const gf_frame_ref* gray, const gf_frame_ref* depth,
                                      gf_feature_obs* out, int cap, int* n_out);
/* trackImage (feature_tracker.h:47) on device images by reference for every sequence: the call above with the list 0 .. batch-1 */
int gf_tracker_track_batch_device_refs(gf_tracker* h, const double* t, const gf_frame_ref* gray, const gf_frame_ref* depth,
                                       gf_feature_obs* out, int cap, int* n_out);
/* trackImage (feature_tracker.h:47), staged: as gf_tracker_prefetch_batch for the listed sequences.  The staged frame remembers its list, and the matching
 * gf_tracker_track_prefetched advances exactly those sequences, its t / out / n_out in the staged order; two staged frames may name different sets.  An empty
 * list is staged as well (its gf_tracker_track_prefetched does nothing), so that prefetch and track calls stay paired. */
int gf_tracker_prefetch_some(gf_tracker* h, int count, const int* seq, const uint8_t* const* gray, int stride,
                             const uint16_t* const* depth, int dstride);

/* FeatureTracker::setPrediction (feature_tracker.cpp:1006-1027): ids[n], xyz[3n] camera-frame points. */
int gf_tracker_set_prediction(gf_tracker* h, int seq, const int* ids, const double* xyz, int n);
/* Region of interest: where in the image a sequence may hold features.  A sequence has either none (the default; every result as without these calls, bit for
 * bit) or a height x width binary image R (on intake non-zero = allowed, 0 = excluded).  With R set, a tracker call for that sequence is
 * FeatureTracker::trackImage (feature_tracker.cpp:103-372) with the first line of setMask() (:58, `mask = cv::Mat(row, col, CV_8UC1, cv::Scalar(255))`) replaced
 * by `mask = R` with R in {0, 255} -- VINS-Mono's `fisheye_mask.clone()`:
 *   1. a tracked point whose rounded pixel has R == 0 is dropped in setMask's walk (in track-count order, after LK and its checks): not kept, no circle painted,
 *      not reported, gone from ids / track_cnt / prev_pts; its id never comes back;
 *   2. new corners are sought in R minus the circles of the kept points: the quality threshold is 0.01 x the largest eigenvalue over THAT set (minMaxLoc with
 *      mask), while the 3 x 3 local-maximum test still looks at excluded neighbours, as goodFeaturesToTrack does;
 *   3. everything else -- LK, the reverse check, the border and grey checks, setPrediction, removeOutliers, depth sampling, velocities, the min-distance
 *      greedy -- is unchanged.  (trackImagebox's filter of the OUTPUT, which keeps boxed features alive inside the tracker, is not what this is.)
 * R belongs to the SEQUENCE, not to a call or a list position; it stays until it is replaced or cleared, and a setter takes effect with the next frame the
 * sequence is given, through every entry point (host, prefetched and device frames, the _some forms, colour and equalize handles alike).  A region that
 * excludes everything is no error: the sequence reports no features.  The table (one bit per pixel) is allocated when the first region of a handle is set; a
 * handle that sets none allocates and launches nothing for it.  Refused with GF_ERR_INVALID, nothing changed: a null handle, seq out of range or named twice
 * in a list, count < 0 or > batch, stride < width.  Like the track calls, one caller thread per handle. */
/* R from a host image, rows `stride` bytes apart (>= width); mask == NULL clears the sequence's region */
int gf_tracker_set_roi(gf_tracker* h, int seq, const uint8_t* mask, int stride);
/* R for the `count` listed sequences from device memory: d_masks = count tight height x width byte images back to back, in list order (a segmentation that
 * lives on the GPU).  Ordered on the handle's stream like the device frame entry points (the masks must be complete when the call is made); returns when the
 * table is written.  d_masks == NULL clears the listed sequences.  Leaves the very bits gf_tracker_set_roi leaves for the same image. */
int gf_tracker_set_roi_some_device(gf_tracker* h, int count, const int* seq, const void* d_masks);
/* The same with the masks where they lie, for the next FeatureTracker::trackImage (feature_tracker.h:47) of each listed sequence: masks[i] = pointer and pitch
 * (>= width, any alignment) of the height x width byte image of seq[i], e.g. a channel or a crop of a segmentation network's output tensor; never written.
 * masks == NULL clears the listed sequences.  Refusals as above plus a null data pointer or a pitch shorter than a row (the message names the list position);
 * leaves the bits of the tight setter. */
int gf_tracker_set_roi_some_device_refs(gf_tracker* h, int count, const int* seq, const gf_frame_ref* masks);
/* *has = whether the sequence has a region in force -- a base region R or a non-empty list of exclusion boxes (below); if so and mask != NULL, that region
 * (R_eff) as 0 / 255 bytes, rows `stride` bytes apart (>= width).  For a sequence without boxes: the stored R, as ever. */
int gf_tracker_get_roi(gf_tracker* h, int seq, uint8_t* mask, int stride, int* has);
/* Exclusion boxes: dynamic objects per sequence and frame, from a detector that runs beside the tracker.  The reference takes darknet_ros_msgs/BoundingBoxes in
 * trackImagebox (feature_tracker.cpp:374), withholds the features strictly inside a rectangle (:565-599, pointPolygonTest(...) > 0) and draws the rectangles
 * (drawTrackbox, :960-975).  Here a box feeds the region of interest: the region in force of a sequence is
 *     R_eff = R_base AND NOT union(boxes),
 * R_base the region of gf_tracker_set_roi* (all allowed if none is set), a box excluding the pixels xmin <= x <= xmax && ymin <= y <= ymax of the frame.  Every
 * float position strictly inside the rectangle rounds to a pixel of that closed box, so every feature the reference would withhold is excluded -- in setMask's
 * walk, on its rounded pixel, as with any region (points 1-3 above with R = R_eff).  Any int32_t is accepted, INT32_MIN and INT32_MAX included; a box is clipped
 * to the frame before any arithmetic; one with xmin > xmax or ymin > ymax excludes nothing.  The boxes belong to the SEQUENCE like R: they hold from the next
 * frame the sequence is given until they are replaced or cleared, through every entry point; gf_tracker_reset_seq keeps them; a base setter leaves them in force
 * over the new base, clearing them restores the base bits.  A handle that never sets boxes allocates, copies and launches exactly what it did without them; the
 * first box setter of a handle allocates a second table (the base words, apart from the words the detector reads) and page-locked staging. */
typedef struct gf_box { int32_t xmin, ymin, xmax, ymax; } gf_box;   /* the four integers of a darknet_ros_msgs/BoundingBox */
typedef char gf_box_is_16_bytes[sizeof(gf_box) == 16 ? 1 : -1];      /* tables of boxes cross the boundary as they lie */
#define GF_MAX_BOXES_PER_SEQ 256   /* a longer list of one sequence is refused */
/* The boxes of the `count` listed sequences for their next frames (trackImagebox's `boxes`, feature_tracker.cpp:374; the filter of :565-599 as a region; what
 * drawTrackbox, :960-975, would draw): those of seq[i] are boxes[first[i] .. first[i + 1]), first = count + 1 offsets.  An empty range clears that sequence;
 * boxes == NULL with first == NULL clears all listed sequences; sequences that are not listed keep what they had.  The boxes are copied into page-locked staging
 * of the handle, and the copy and ONE kernel launch for the whole list (each listed sequence's words of R_eff into the table the detector reads) are ordered on
 * the handle's stream ahead of the next track call: no stream synchronisation, no device-to-host copy.  (A second box or base setter before the next track call
 * waits for the first one's kernel, whose staging it reuses.)  Refused with GF_ERR_INVALID, the message naming the list position, and nothing changed: a null
 * handle, count < 0 or > batch, a sequence out of range or named twice, first[0] != 0 or a decreasing first, a range longer than GF_MAX_BOXES_PER_SEQ,
 * boxes == NULL with a non-empty range, exactly one of first and boxes NULL with count > 0. */
int gf_tracker_set_boxes_some(gf_tracker* h, int count, const int* seq, const int* first, const gf_box* boxes);
/* the boxes in force for seq (trackImagebox's list, feature_tracker.cpp:374, :565-599, :960-975): *n of them, the first min(*n, cap) into boxes (may be NULL
 * with cap == 0) */
int gf_tracker_get_boxes(gf_tracker* h, int seq, gf_box* boxes, int cap, int* n);
/* The composition as a building block on host buffers (copies in, runs the tracker's packing and composing kernels, copies out; synchronous) -- the region
 * trackImagebox's filter (feature_tracker.cpp:374, :565-599; the rectangles of :960-975) leaves, for `batch` frames of height x width, any width >= 1 and
 * height >= 1: the boxes of frame b are boxes[first[b] .. first[b + 1]), each list at most GF_MAX_BOXES_PER_SEQ long; base_masks is NULL (all allowed) or `batch`
 * tight height x width byte images back to back (non-zero = allowed); out_masks: `batch` tight images of 0 / 255. */
int gf_roi_boxes_batch(int batch, int width, int height, const int* first, const gf_box* boxes, const uint8_t* base_masks, uint8_t* out_masks);
/* Parameters per sequence: what the reference keeps per FeatureTracker object (MAX_CNT, MIN_DIST, FLOW_BACK, depth_cam, m_camera; feature_tracker.h:76-98).
 * A sequence that was never set runs with the handle's gf_tracker_cfg, every result as without these calls, bit for bit.  With its parameters set, a tracker
 * call for that sequence is FeatureTracker::trackImage of an object constructed with them: setMask's circles and goodFeaturesToTrack's minimum distance use its
 * min_dist, it tops up to its max_cnt, runs the reverse check or not by its flow_back, liftProjective / spaceToPlane (gf_tracker_set_prediction) and the
 * velocities use its camera, and the output packing and the "depth_cam set but no depth image" rule use its depth_cam -- through every entry point (host,
 * prefetched and device frames, the _some forms, region-of-interest, colour and equalize handles alike), in the launches it shares with its neighbours.  On the
 * host entry points the depth[i] of a listed sequence with depth_cam == 0 is not read and may be NULL.
 * The handle's cfg is also the capacity: 1 <= max_cnt <= cfg.max_cnt (the point arrays are that wide), cfg.min_dist <= min_dist <= 128 (the handle's min_dist
 * sized the selection grid and the sort area when it was created), fx, fy > 0, flow_back and depth_cam 0 or 1.  So a mixed handle is created with the largest
 * count and the tightest spacing of its fleet, and allocates nothing further for the point tables.  Equalize and pixel_format have their own setter (gf_tracker_set_seq_format), width and height theirs (gf_tracker_set_seq_size).
 * The parameters are fixed while a sequence holds tracking state, as they are in the reference after construction: once the sequence has taken a frame the
 * setter is refused until gf_tracker_reset_seq.  The tables (one circle table row per sequence, two small lists per call) are allocated when the first
 * parameters of a handle are set; a handle that sets none allocates and launches nothing for them.  Refused with GF_ERR_INVALID, a message that names the
 * field, and nothing changed: a null handle, seq out of range, a value outside the limits above, a sequence that has taken a frame, a sequence that a
 * frame staged by gf_tracker_prefetch_* lists (setter and gf_tracker_reset_seq alike: gf_tracker_track_prefetched consumes it first).  One caller thread per
 * handle, between frames. */
typedef struct gf_tracker_seq_cfg {
    int max_cnt, min_dist, flow_back, depth_cam;
    double fx, fy, cx, cy, k1, k2, p1, p2;
} gf_tracker_seq_cfg;
/* c == NULL: back to the handle's cfg */
int gf_tracker_set_seq_cfg(gf_tracker* h, int seq, const gf_tracker_seq_cfg* c);
/* what is in force for seq (the handle's values for a sequence that was never set) */
int gf_tracker_get_seq_cfg(gf_tracker* h, int seq, gf_tracker_seq_cfg* out);
/* The sequence as it was after gf_tracker_create -- no tracks, n_id = 0, no previous frame, no pending prediction, prev_time = 0 -- for a slot that another
 * unit takes over.  Keeps the sequence's parameters and its region of interest (they are settings), allows gf_tracker_set_seq_cfg again, touches no other
 * sequence. */
int gf_tracker_reset_seq(gf_tracker* h, int seq);
/* A pixel format and an equalise switch per sequence: what the reference's node does per camera ahead of trackImage, cv_bridge::toCvCopy(msg, MONO8) and the
 * CLAHE of getImageFromMsg (rosNodeTest.cpp:238-261).  A sequence that was never set runs with the handle's gf_tracker_cfg.pixel_format / equalize, and a
 * handle on which the setter is never called allocates, copies, records and launches exactly what it did without it.  With a format of its own, a tracker call
 * for that sequence gives the bits of a handle created with cfg.pixel_format = pixel_format, cfg.equalize = equalize for the same frames -- observations, ids,
 * gf_tracker_get_state, the track image -- through every entry point that takes frames, in the launches it shares with its neighbours: one conversion (two
 * launches at the most, whatever the formats), one CLAHE launch over the equalised sequences, one pyramid.  A MONO8 sequence without equalisation is read by
 * the pyramid where the caller's frame lies; it is not copied.
 * Layouts.  Host list entry points: the row step of listed sequence i is host_stride if non-zero, otherwise the call's `stride`, and must be >= width x bytes
 * per pixel of THAT sequence's format.  Tight device entry points: the frames lie back to back in list order, frame i has height x width x bytes per pixel of
 * seq[i] bytes, so its offset is the sum of the frames listed before it.  _refs entry points: pitch >= width x bytes per pixel of that sequence's format.
 * Depth frames are untouched.  A call with a too-short stride or pitch is refused naming the list position, and changes nothing.
 * A setting, like gf_tracker_seq_cfg: fixed while the sequence holds tracking state (refused once it has taken a frame, until gf_tracker_reset_seq, which
 * keeps it), refused while any frame staged by gf_tracker_prefetch_* is waiting (the staging buffers may have to grow).  The first setter that needs them
 * allocates the conversion and equalisation buffers and LUTs for the batch and grows the staging buffers to the widest format set so far; GF_ERR_HIP and nothing
 * changed if that fails.  Refused with GF_ERR_INVALID, a message that names the field, and nothing changed: a null handle, seq out of range, a pixel_format
 * gf_tracker_create refuses, equalize not 0 / 1, host_stride < 0 or non-zero and below a row of the format.
 * gf_tracker_stats.ms_convert / ms_equalize grow on the calls that convert / equalise at least one listed sequence, and only on those. */
typedef struct gf_tracker_seq_format {
    int pixel_format;  /* GF_PIX_*: the format of every frame this sequence is given */
    int equalize;      /* 0 / 1: CLAHE (clip 40, 8 x 8) on this sequence's MONO8 frame before the pyramid */
    int host_stride;   /* bytes per row of this sequence's HOST frames on the list entry points; 0 = the call's `stride` */
} gf_tracker_seq_format;
/* rosNodeTest.cpp:238-261 per sequence.  f == NULL: back to the handle's gf_tracker_cfg.pixel_format / equalize, host_stride 0 */
int gf_tracker_set_seq_format(gf_tracker* h, int seq, const gf_tracker_seq_format* f);
/* rosNodeTest.cpp:238-261 per sequence: what is in force for seq (the handle's values for a sequence that was never set) */
int gf_tracker_get_seq_format(gf_tracker* h, int seq, gf_tracker_seq_format* out);
/* A frame size per sequence: `row`, `col` of FeatureTracker::trackImage (feature_tracker.cpp:108-109) for the sequence, where they are not the handle's.  A
 * sequence that was never set has gf_tracker_cfg.width x height, and a handle on which the setter is never called allocates, copies, records and launches
 * exactly what it did without it.  With a size of its own, a tracker call for that sequence is trackImage on frames of width x height: the observations, ids,
 * gf_tracker_get_state and the track image are the bits of a handle created with cfg.width = width, cfg.height = height and otherwise the same settings -- the
 * pyramid's levels, borders and stop rule, inBorder, the grey check and the depth sample, setMask's image, the detector's strips and bands and the selection
 * grid -- in the launches it shares with its neighbours: LK, the detector, the selection and the region kernels serve every size in one launch
 * (gf_tracker_stats.lk_launches is that of a homogeneous call); the pyramid, the conversion, CLAHE and the track image run once per distinct size among the
 * listed sequences, the pyramid on the route a handle of that size takes (gf_tracker_stats.pyr_*).
 * The handle's cfg is the capacity, as with max_cnt: 32 <= width <= cfg.width, 32 <= height <= cfg.height, width % 4 == 0; the sequence's pyramid slots, its
 * row of the region table and its share of the frame buffers stay where they are and as large as they are.  At most GF_MAX_SEQ_SIZES distinct sizes are in
 * force on a handle at a time, the handle's own included.  (0, 0) returns the sequence to the handle's size.
 * Everything of the sequence that is an image has its size.  Gray and depth frames: on the host list entry points and gf_tracker_prefetch_some `stride` (or the
 * sequence's host_stride) must be at least a row of its own width and format and `dstride` at least its own width; on the tight device entry points the frames
 * lie back to back in list order, frame i has its own height x width x bytes per pixel (depth: x 2), so its offset is the sum of the frames listed before it;
 * on the _refs entry points the pitch must be at least a row of its own width.  The region setters take masks of the sequence's size (tight device lists at
 * prefix-sum offsets, _refs masks with a pitch of at least the own width), gf_tracker_get_roi returns one, the boxes are clipped to it, and
 * gf_tracker_track_image* work on a picture of it.  A call with a shorter stride or pitch is refused naming the list position, and changes nothing.  A tight
 * device list laid out otherwise (at the handle's size, say) cannot be told from a right one, since a pointer carries no size: the layout is the caller's.
 * A setting, like gf_tracker_seq_cfg: fixed while the sequence holds tracking state (refused once it has taken a frame, until gf_tracker_reset_seq, which
 * keeps it), refused while a frame staged by gf_tracker_prefetch_* lists the sequence and while the sequence has a region of interest, an image of the old size
 * (clear it first); exclusion boxes stay, clipped to and composed in the new frame.  On a handle that never gave a sequence a size, (0, 0) and the handle's
 * own size change nothing and are accepted in every state.  The first setter of a handle allocates the table of sizes and the tables of a call; GF_ERR_HIP and nothing changed
 * if that fails.  Refused with GF_ERR_INVALID, a message that names the field, and nothing changed: a null handle, seq out of range, a size outside the
 * limits, a ninth distinct size, and the state conditions above. */
#define GF_MAX_SEQ_SIZES 8
int gf_tracker_set_seq_size(gf_tracker* h, int seq, int width, int height);
/* feature_tracker.cpp:108-109 per sequence: the size in force for seq (the handle's for a sequence that was never set) */
int gf_tracker_get_seq_size(gf_tracker* h, int seq, int* width, int* height);
/* A camera model per sequence: what FeatureTracker::readIntrinsicParameter (feature_tracker.cpp:745-759) gets from CameraFactory::generateCameraFromYamlFile --
 * camodocal's PINHOLE (PinholeCamera), MEI (CataCamera) or KANNALA_BRANDT (EquidistantCamera); PINHOLE_FULL and SCARAMUZZA need the wide struct gf_camera_model_ex below.  liftProjective
 * (undistortedPts, feature_tracker.cpp:797-808) and spaceToPlane (setPrediction, :1006-1027) of the sequence then are that model's: PinholeCamera.cc:450-542,
 * CataCamera.cc:556-659, EquidistantCamera.cc:428-461 with backprojectSymmetric (:716-818), in double precision (csrc/gf_camera_models.hpp; DESIGN.md
 * section 4, "Camera models").  Pixel coordinates, ids, track counts and depths do not depend on the model.
 *   proj   PINHOLE fx fy cx cy | MEI gamma1 gamma2 u0 v0 | KANNALA_BRANDT mu mv u0 v0
 *   dist   PINHOLE k1 k2 p1 p2 | MEI k1 k2 p1 p2        | KANNALA_BRANDT k2 k3 k4 k5
 * Refused wherever a model is taken (GF_ERR_INVALID, the message naming the field): a model that is none of the three, reserved != 0, a value that is not
 * finite, proj[0] or proj[1] <= 0, xi < 0 (MEI), and a KANNALA_BRANDT set in which a zero coefficient precedes a non-zero one (k3 = 0 with k5 != 0, say): the
 * reference divides by zero for such a set. */
enum { GF_CAMERA_PINHOLE = 0, GF_CAMERA_MEI = 1, GF_CAMERA_KANNALA_BRANDT = 2 };
typedef struct gf_camera_model {
    int32_t model;      /* GF_CAMERA_PINHOLE 0, GF_CAMERA_MEI 1, GF_CAMERA_KANNALA_BRANDT 2 */
    int32_t reserved;   /* 0 */
    double proj[4];     /* fx fy cx cy | gamma1 gamma2 u0 v0 | mu mv u0 v0 */
    double dist[4];     /* k1 k2 p1 p2 | k1 k2 p1 p2        | k2 k3 k4 k5 */
    double xi;          /* MEI only */
} gf_camera_model;
typedef char gf_camera_model_is_80_bytes[sizeof(gf_camera_model) == 80 ? 1 : -1];
/* The camera of seq (feature_tracker.cpp:745-759).  A setting like gf_tracker_seq_cfg: refused once the sequence has taken a frame (until gf_tracker_reset_seq,
 * which keeps it) and while a frame staged by gf_tracker_prefetch_* lists it.  With GF_CAMERA_PINHOLE the call is gf_tracker_set_seq_cfg with the eight camera
 * fields replaced.  With another model the camera fields of the sequence's gf_tracker_seq_cfg stay stored, unused until a pinhole is set again; the sequence's
 * points are lifted by ONE kernel launch per tracker call behind the corner selection, for all listed sequences with such a model (environment
 * GF_CAMERA_LIFT_HOST=1, read by gf_tracker_create: on the host instead, with the same formulas), and the lifted pairs come back with the call's last copies:
 * no further synchronisation.  Pinhole sequences keep their host lift bit for bit, and a handle on which no such model is set allocates, copies and launches
 * what it did without these calls. */
int gf_tracker_set_seq_camera(gf_tracker* h, int seq, const gf_camera_model* cam);
/* feature_tracker.cpp:745-759: the camera in force for seq; ahead of any setter the pinhole of the sequence's gf_tracker_seq_cfg */
int gf_tracker_get_seq_camera(gf_tracker* h, int seq, gf_camera_model* out);
/* liftProjective (PinholeCamera.cc:450-510, CataCamera.cc:556-626, EquidistantCamera.cc:428-442) as a building block, through the tracker's kernel: sequence b
 * of `batch` has camera cams[b] and the points uv[first[b] .. first[b + 1]) (float pixel pairs; first: batch + 1 offsets from 0, not decreasing).  rays: 3
 * doubles per point, the ray P (may be NULL); un: the float pair (float)(P.x / P.z), (float)(P.y / P.z) of feature_tracker.cpp:803-805.  Every point takes a
 * bounded number of steps whatever its coordinates.  Host arrays (copies in, one launch, copies out; synchronous). */
int gf_camera_lift_batch(const gf_camera_model* cams, int batch, const int* first, const float* uv, double* rays, float* un);
/* The same lift (feature_tracker.cpp:797-808) on device arrays: uv, rays (may be NULL) and un are device pointers of the current device; cams and first stay
 * host tables.  One launch on `stream` (a hipStream_t, NULL = the null stream); returns when it has run (the checked cameras travel in staging of the call). */
int gf_camera_lift_batch_device(const gf_camera_model* cams, int batch, const int* first, const float* d_uv, double* d_rays, float* d_un, void* stream);
/* spaceToPlane (PinholeCamera.cc:520-542, CataCamera.cc:636-659, EquidistantCamera.cc:451-461) on the host, what setPrediction uses: xyz 3 doubles per
 * point, uv 2 doubles per point, sequences and offsets as above. */
int gf_camera_project_batch(const gf_camera_model* cams, int batch, const int* first, const double* xyz, double* uv);
/* A camodocal calibration file (CameraFactory::generateCameraFromYamlFile, CameraFactory.cc; keys as PinholeCamera.cc:145-183, CataCamera.cc:160-202,
 * EquidistantCamera.cc:146-182): model_type (missing: PINHOLE), projection_parameters, distortion_parameters, mirror_parameters.xi.  A missing numeric key reads
 * as 0 like every cv::FileNode, so a missing focal parameter is refused by name; PINHOLE_FULL and SCARAMUZZA are refused by name, pointing at gf_camera_from_yaml_ex. */
int gf_camera_from_yaml(const char* calib_file, gf_camera_model* out);
/* All five camodocal models: the three above and PINHOLE_FULL (PinholeFullCamera: OpenCV's rational model k1..k6, p1, p2 -- the only one that holds a calibration
 * with a k3 or the 8-coefficient factory calibration of a Kinect-class camera) and SCARAMUZZA (OCAMCamera, OCamCalib), which the 80-byte struct cannot carry.
 * liftProjective and spaceToPlane: PinholeFullCamera.cc:535-607, :623-645 with :754-780; ScaramuzzaCamera.cc:599-622, :632-655 (csrc/gf_camera_models.hpp).
 *   PINHOLE_FULL  liftProjective is the reference's loop as it runs: nine passes, no error test (its test can never end the loop) -- the ninth iterate, not the
 *                 true inverse.
 *   SCARAMUZZA    the reference's arithmetic with its quirks: the ray is (xc, -z) of the uncorrected xc with z a polynomial in the norm of the affine-corrected
 *                 xc; a ray on the axis projects to a non-finite pixel.
 * Fields a model does not use are not read.  Refused (GF_ERR_INVALID, the message naming the field): reserved != 0, a model outside 0 .. 4, a value that is read
 * and is not finite, PINHOLE_FULL with fx or fy <= 0, SCARAMUZZA with ac - ad * ae == 0 (the reference divides by it), and for models 0-2 what gf_camera_model
 * is refused for.  The calls below behave like the ones without _ex for models 0-2, bit for bit; those keep refusing models 3 and 4. */
enum { GF_CAMERA_PINHOLE_FULL = 3, GF_CAMERA_SCARAMUZZA = 4 };   /* valid in gf_camera_model_ex only */
typedef struct gf_camera_model_ex {
    int32_t model, reserved;      /* reserved 0 */
    double proj[4];               /* as gf_camera_model | PINHOLE_FULL fx fy cx cy | SCARAMUZZA: not read */
    double dist[8];               /* models 0-2: the first four as gf_camera_model | PINHOLE_FULL k1 k2 p1 p2 k3 k4 k5 k6 */
    double xi;                    /* MEI only */
    double poly[5];               /* SCARAMUZZA poly_parameters p0..p4 */
    double inv_poly[20];          /* SCARAMUZZA inv_poly_parameters p0..p19 */
    double affine[5];             /* SCARAMUZZA affine_parameters ac ad ae cx cy */
} gf_camera_model_ex;
typedef char gf_camera_model_ex_is_352_bytes[sizeof(gf_camera_model_ex) == 352 ? 1 : -1];
/* gf_tracker_set_seq_camera for any of the five models.  PINHOLE_FULL sequences are lifted by the same one launch per call as MEI and KANNALA_BRANDT ones,
 * and so are SCARAMUZZA sequences under GF_CAMERA_LIFT_HOST=0; by default those are lifted on the host (gf_tracker_get_camera_lift_stats below). */
int gf_tracker_set_seq_camera_ex(gf_tracker* h, int seq, const gf_camera_model_ex* cam);
/* gf_tracker_get_seq_camera for any model; gf_tracker_get_seq_camera itself refuses a sequence whose camera is PINHOLE_FULL or SCARAMUZZA by name */
int gf_tracker_get_seq_camera_ex(gf_tracker* h, int seq, gf_camera_model_ex* out);
/* Where the lift runs, per model, by what was measured (profiles/camera_wide_measure.json): MEI, KANNALA_BRANDT and PINHOLE_FULL sequences on the device,
 * SCARAMUZZA sequences -- a fifth-degree polynomial per point -- on the host, like PINHOLE ones.  GF_CAMERA_LIFT_HOST (read by gf_tracker_create) overrides it
 * for every model: 1 all on the host, 0 all on the device.  A sequence lifted on the host is not listed for the kernel; a call lists either some sequence
 * and has ONE launch of camera_lift_kernel, whatever the mix of models, or none and has no launch.
 * The lift's own counters (gf_tracker_stats keeps its layout), each may be NULL: launches of camera_lift_kernel by this handle, and listed sequences those
 * launches lifted, summed.  A stereo sequence (gf_tracker_set_seq_stereo) whose RIGHT camera is lifted on the device is one more list entry of the same launch
 * and counts as one more listed sequence: `sequences` sums left and right lifts, and a call in which only right cameras are lifted still has its one launch.
 * gf_tracker_reset_stats zeroes them. */
int gf_tracker_get_camera_lift_stats(gf_tracker* h, long long* launches, long long* sequences);
/* gf_camera_lift_batch, gf_camera_lift_batch_device and gf_camera_project_batch with cameras of any of the five models */
int gf_camera_lift_batch_ex(const gf_camera_model_ex* cams, int batch, const int* first, const float* uv, double* rays, float* un);
int gf_camera_lift_batch_device_ex(const gf_camera_model_ex* cams, int batch, const int* first, const float* d_uv, double* d_rays, float* d_un, void* stream);
int gf_camera_project_batch_ex(const gf_camera_model_ex* cams, int batch, const int* first, const double* xyz, double* uv);
/* gf_camera_from_yaml for all five models; model_type is compared without regard to case as CameraFactory.cc:111-129 does.  PINHOLE_FULL keys as
 * PinholeFullCamera.cc:209-249 (distortion_parameters k1..k6 p1 p2, projection_parameters fx fy cx cy; a missing fx or fy is refused by name), SCARAMUZZA keys
 * as ScaramuzzaCamera.cc:64-105 (poly_parameters p0..p4, inv_poly_parameters p0..p19, affine_parameters ac ad ae cx cy). */
int gf_camera_from_yaml_ex(const char* calib_file, gf_camera_model_ex* out);
/* Depth registration: the raw frame of a depth camera brought to the colour camera on the device -- what the camera driver's `align` filter does on the host for
 * /camera/aligned_depth_to_color/image_raw, the topic every shipped configuration subscribes to (config/realsense/m2dgrp.yaml:23), as a definition of this
 * repository (csrc/gf_depth_reg.hpp; DESIGN.md section 4, "Depth registration").  width x height u16 counts of `scale` metres each, seen through the undistorted
 * pinhole fx fy cx cy, are lifted, moved by P_colour = R P_depth + T (R row-major, T in metres) and projected through the colour PINHOLE with its distortion; each
 * depth pixel covers the colour pixels whose centre lies in the half-open box between the images of its two corners (nothing if that box is wider or higher than
 * 8 pixels), with floor(Pz / 0.001 + 0.5) millimetres along the colour camera's axis; a colour pixel takes the smallest value that reaches it, 0 (no
 * measurement) if none does.  The identity registration (same size and intrinsics, R = I, T = 0, scale = 0.001) returns its input.  A count of 0, a point not in
 * front of the colour camera, a coordinate that is not finite and a value outside 1 .. 65535 contribute nothing.
 * Refused wherever a registration is taken (GF_ERR_INVALID, the message naming the field): width or height outside 8 .. 4096, a value that is not finite, fx, fy
 * or scale <= 0, an R with an entry of R R^T - I beyond 1e-6 or with det R <= 0.  Out of scope: a colour camera other than GF_CAMERA_PINHOLE or, through the _ex calls and
 * gf_tracker_set_seq_camera_ex, GF_CAMERA_PINHOLE_FULL (refused by name), a distorted depth stream, depth in floating point. */
typedef struct gf_depth_reg {
    int32_t width, height;   /* of the raw depth frame */
    double fx, fy, cx, cy;   /* the depth stream's pinhole (depth streams are rectified) */
    double scale;            /* metres per count: 0.001 for millimetres, 0.0001 for a D405, 0.00025 for an L515 */
    double R[9], T[3];       /* depth -> colour: P_colour = R P_depth + T, R row-major, T in metres */
} gf_depth_reg;
typedef char gf_depth_reg_is_144_bytes[sizeof(gf_depth_reg) == 144 ? 1 : -1];
/* The registration as a building block, through the tracker's two kernels: entry b of `batch` has the raw frame d_src[b] (reg[b].height rows of reg[b].width
 * counts), the registration reg[b], the colour camera colour[b] (GF_CAMERA_PINHOLE) of colour_wh[2 b] x colour_wh[2 b + 1] pixels (each 8 .. 4096), and the
 * registered frame d_dst[b] of that size.  reg, colour and colour_wh are host tables; sources and destinations are device frames by pointer and pitch (both
 * even, pitch >= 2 x the width; a refusal names the entry).  d_dst IS WRITTEN, as the dst of gf_tracker_track_image_some_device is: 2 x colour width bytes of each
 * row, never a byte beyond them.  Entries may have different sizes; the call is two launches on `stream` (a hipStream_t, NULL = the null stream) whatever the
 * batch, and returns when they have run.  The z-buffer is staging of the library that grows with the largest call and is left primed for the next one. */
int gf_depth_register_batch_device(const gf_frame_ref* d_src, const gf_depth_reg* reg, const gf_camera_model* colour, const int* colour_wh,
                                   const gf_frame_ref* d_dst, int batch, void* stream);
/* The same on host frames by pointer and pitch (copies in, the two launches, copies out; synchronous): for tests and callers without device frames */
int gf_depth_register_batch(const gf_frame_ref* src, const gf_depth_reg* reg, const gf_camera_model* colour, const int* colour_wh, const gf_frame_ref* dst, int batch);
/* The two calls above with colour cameras that are GF_CAMERA_PINHOLE or GF_CAMERA_PINHOLE_FULL (every other model is refused by name).  For a PINHOLE_FULL entry
 * the projection is the tail of that model's spaceToPlane (PinholeFullCamera.cc:630-644 with :754-780) in the place of the pinhole's; footprints, the 8-pixel
 * bound, the z-buffer and the second kernel are the same.  Still two launches whatever the mix; PINHOLE entries come out as from the calls above, byte for byte. */
int gf_depth_register_batch_device_ex(const gf_frame_ref* d_src, const gf_depth_reg* reg, const gf_camera_model_ex* colour, const int* colour_wh,
                                      const gf_frame_ref* d_dst, int batch, void* stream);
int gf_depth_register_batch_ex(const gf_frame_ref* src, const gf_depth_reg* reg, const gf_camera_model_ex* colour, const int* colour_wh, const gf_frame_ref* dst, int batch);
/* The registration of seq; reg == NULL clears it.  With one set, the `depth` entry of the sequence on gf_tracker_track_some_device_refs / _track_batch_device_refs
 * is the RAW frame of the depth camera -- reg->height rows of reg->width counts, pointer and pitch even, pitch >= 2 x reg->width; a call that breaks this is
 * refused naming the list position -- and the call registers it to the sequence's colour camera (the PINHOLE of its gf_tracker_seq_cfg, or the PINHOLE_FULL
 * camera gf_tracker_set_seq_camera_ex gave it, at its frame size in force) into a frame of the handle before anything samples depth: two launches per call for all such sequences, whatever their number and sizes.  LK and the
 * corner selection then sample that frame, so the call's results are those of the same call on frames registered beforehand by gf_depth_register_batch_device.
 * A sequence whose depth_cam is 0 may carry a registration; it is never run.  Every other entry point (host images, tight device lists, prefetch) refuses a
 * call with depth that lists such a sequence (GF_ERR_INVALID, the message naming the entry point and the sequence, nothing changed): host images would put the
 * raw frame on the bus.  Without depth, and for lists without such a sequence, they behave as before.
 * A setting like gf_tracker_set_seq_size: refused once the sequence has taken a frame (until gf_tracker_reset_seq, which keeps it), while a frame staged by
 * gf_tracker_prefetch_* lists it, and while the sequence's camera is neither GF_CAMERA_PINHOLE nor GF_CAMERA_PINHOLE_FULL (gf_tracker_set_seq_camera / _ex; those
 * setters in turn refuse another model while a registration is set).  The first setter of a handle allocates the registered frames and the z-buffer at the handle's capacity (cfg.width x cfg.height
 * per sequence) and the call's table; GF_ERR_HIP and nothing changed if that fails.  A handle on which it is never called allocates, copies and launches
 * exactly what it did without it. */
int gf_tracker_set_seq_depth_reg(gf_tracker* h, int seq, const gf_depth_reg* reg);
/* *has = whether seq has a registration; if so and out != NULL, the registration as it was set */
int gf_tracker_get_seq_depth_reg(gf_tracker* h, int seq, gf_depth_reg* out, int* has);
/* The registration's own counters (gf_tracker_stats keeps its layout), each may be NULL: kernel launches (two per tracker call that registered a frame), frames
 * registered, and the hipEvent time of the two kernels, summed.  gf_tracker_reset_stats zeroes them. */
int gf_tracker_get_depth_reg_stats(gf_tracker* h, long long* launches, long long* frames, double* kernel_ms);
/* rejectWithF: FeatureTracker::rejectWithF (feature_tracker.cpp:711-743; F_threshold, parameters.cpp:201), the epipolar outlier test between LK and the back
 * end, as a definition of this repository (csrc/gf_reject_f.hpp; DESIGN.md section 4, "rejectWithF"): cv::findFundamentalMat(FM_RANSAC) cannot be restated bit
 * for bit.  The points LK kept are lifted with the sequence's camera to virtual pixels FOCAL_LENGTH X / Z + width / 2, FOCAL_LENGTH Y / Z + height / 2
 * (:722-729); GF_REJECT_F_HYPOTHESES eight-point models are drawn by a counter-based hash, solved by Hartley normalisation and Gaussian elimination with full
 * pivoting in double, and scored by the larger of the two squared epipolar distances against f_threshold^2; the outliers of the model with the most inliers
 * (ties: the first) lose their status.  Fewer than 8 candidates, or no valid model (a camera at rest with bit-identical points): nothing is rejected -- OpenCV
 * would return an empty matrix and the reference would drop every point.  Host (GF_REJECT_F_HOST=1, read at gf_tracker_create), kernel and the numpy
 * restatement of the tests give the same bytes. */
#define GF_REJECT_F_HYPOTHESES 512
#define GF_REJECT_F_MAX_PAIRS 1024   /* pairs of one set of the building blocks; points of a sequence whose switch is on */
/* Field order: enable, seed, f_threshold, focal_length -- the two 32-bit fields first, 24 bytes without padding.  Initialise by field name. */
typedef struct gf_reject_f_cfg {
    int32_t enable;          /* 0: off (the reference leaves the call commented out at feature_tracker.cpp:183 and :454) */
    uint32_t seed;           /* of the draws; mixed with the number of frames the sequence has taken since create / gf_tracker_reset_seq */
    double f_threshold;      /* F_THRESHOLD in virtual pixels (parameters.cpp:201; 1.0 in every shipped configuration): finite, > 0 */
    double focal_length;     /* FOCAL_LENGTH of the virtual camera (parameters.h:23); 0 means 460 */
} gf_reject_f_cfg;
typedef struct gf_reject_f_result {   /* of one set */
    int32_t m;          /* candidates: pairs with status 1 and finite coordinates */
    int32_t rejected;   /* status bytes cleared, pairs with a non-finite coordinate included */
    int32_t winner;     /* the winning hypothesis, -1: none (m < 8 or every hypothesis void) */
    int32_t inliers;    /* its inliers */
} gf_reject_f_result;
typedef struct gf_reject_f_stats {   /* gf_tracker_stats keeps its layout */
    long long launches;     /* of reject_f_kernel: one per tracker call that lists a sequence with the switch on and 8 or more points, two where a predicted sequence fell back to the three-level LK (:131-132) */
    long long sequences;    /* sequence frames the stage ran on */
    long long candidates, rejected;
    long long no_model;     /* of those with 8 or more candidates: every hypothesis void, nothing rejected */
    double kernel_ms;       /* hipEvent time of the kernel, summed (0 under GF_REJECT_F_HOST=1) */
} gf_reject_f_stats;
/* rejectWithF of seq (feature_tracker.cpp:711-743); c == NULL or c->enable == 0 turns it off.  From then on every entry point that takes frames (host images,
 * tight device lists, _refs, prefetched, _some, _sized) applies the stage to the sequence's points behind LK, ahead of track_cnt++ and setMask as the reference
 * orders them at :170-186: one more launch on the tracking stream per call whatever the number of such sequences, which rewrites the status bytes before the
 * host reads them.  Allowed between frames at any time.  Refused (GF_ERR_INVALID, the message naming the field, nothing changed): f_threshold not finite or
 * <= 0, focal_length not finite or < 0, a sequence that a frame staged by gf_tracker_prefetch_* lists; GF_ERR_CAPACITY on a handle whose sequences hold more
 * than GF_REJECT_F_MAX_PAIRS points.  The first setter of a handle that turns a switch on allocates the call's table; a handle on which it is never called
 * allocates, copies and launches exactly what it did without it. */
int gf_tracker_set_seq_reject_f(gf_tracker* h, int seq, const gf_reject_f_cfg* c);
/* the configuration of seq as it was set; enable == 0 and zeros if it is off (feature_tracker.cpp:711-743) */
int gf_tracker_get_seq_reject_f(gf_tracker* h, int seq, gf_reject_f_cfg* out);
/* the stage's own counters (feature_tracker.cpp:711-743); gf_tracker_reset_stats zeroes them */
int gf_tracker_get_reject_f_stats(gf_tracker* h, gf_reject_f_stats* out);

/* ---- a right camera per sequence: the stereo branch of trackImage (feature_tracker.cpp:259-303, kept there as VINS-Fusion wrote it, commented out; its place is
 * behind undistortedPts / ptsVelocity of the left, :210-211, and ahead of the roll-over, :307-312).  DESIGN.md section 4, "Stereo", is the definition. */
typedef struct gf_stereo_cfg {
    int enable;                 /* 1: the sequence has a right camera (stereo_cam, feature_tracker.cpp:751-752) */
    int reserved;               /* must be 0 */
    gf_camera_model_ex right;   /* m_camera[1] (:298): the camera cur_right_pts is lifted through */
} gf_stereo_cfg;
typedef struct gf_stereo_stats {
    long long calls;            /* tracker calls that ran the stage for at least one sequence */
    long long launches;         /* launches of the stereo kernel (one per such call) */
    long long points;           /* points submitted: cur_pts of every sequence and frame the stage ran for (:273) */
    long long matched;          /* points kept: entries of ids_right (:286-288) */
    long long right_pyramids;   /* right pyramids built */
} gf_stereo_stats;
/* The switch and the right camera of seq, before its first frame like the other per-sequence setters (c == NULL or enable == 0: off).  A stereo sequence takes
 * its right frame (`_img1`, :259) where the reference's travels: the second gf_frame_ref of its list position on gf_tracker_track_some_device_refs /
 * gf_tracker_track_batch_device_refs, 8-bit, of the sequence's own size, with any pointer or pitch (the "even" rule stays for depth entries).  An entry with
 * data == NULL is `_img1.empty()`: the stage is skipped for that frame and the right-hand state stays as it is, so the next frame with a right image takes its
 * velocities against the map of the last frame that ran the stage, over the newest dt.  With a right frame the call returns the left observations as ever, then
 * one observation per entry of ids_right in that order: camera_id 1, v = (x_un_right, y_un_right, 1, u_right, v_right, vx_right, vy_right, -2.4); n_out counts
 * both and the capacity rule holds for the sum.  Forward LK from the left frame to the right on all of cur_pts and, with the sequence's own FLOW_BACK, the
 * reverse pass and the 0.5 px test (:273-284) run in ONE launch per call for all its stereo sequences, behind the corner selection; the right camera's lift
 * (:298) takes the route its model takes on the left: PINHOLE on the host, the others as one more list entry of the call's camera_lift_kernel launch
 * (GF_CAMERA_LIFT_HOST is honoured).  A sequence that equalises equalises both eyes (rosNodeTest.cpp:256-261).  On the host-image, tight and prefetch entry points a stereo sequence listed without a second image is a mono frame; with one the
 * call is refused by name, nothing changed.  Refused by name, nothing changed: a sequence that has taken a frame or is listed by a staged one, reserved != 0,
 * a right camera gf_camera_model_ex's rules refuse, stereo together with depth_cam or a depth registration, and a pixel format other than GF_PIX_MONO8.
 * gf_tracker_set_seq_cfg / _format / _depth_reg refuse the same
 * combinations from their side.  removeOutliers and setPrediction act on the left lists only; gf_tracker_reset_seq clears the right-hand state.  The first
 * setter of a handle that turns a switch on allocates the right pyramids and the call's tables; a handle on which it is never called allocates, copies and
 * launches exactly what it did without it. */
int gf_tracker_set_seq_stereo(gf_tracker* h, int seq, const gf_stereo_cfg* c);
/* the configuration of seq as it was set; enable == 0 and zeros if it is off (feature_tracker.cpp:259) */
int gf_tracker_get_seq_stereo(gf_tracker* h, int seq, gf_stereo_cfg* out);
/* the stage's own counters (feature_tracker.cpp:259-303); gf_tracker_reset_stats zeroes them */
int gf_tracker_get_stereo_stats(gf_tracker* h, gf_stereo_stats* out);
/* The switch and the right camera from a config file (feature_tracker.cpp:259; parameters.cpp:424-436): `num_of_cam: 2` turns the switch on and `cam1_calib` names
 * the right camera's calibration file beside the config file, read as gf_camera_from_yaml_ex reads one; any other num_of_cam: enable == 0 and zeros, no second
 * file is read.  GF_ERR_INVALID, naming the file and the key: num_of_cam 2 without cam1_calib, a calibration file that cannot be read or that
 * gf_camera_from_yaml_ex refuses. */
int gf_stereo_from_yaml(const char* config_file, gf_stereo_cfg* out);
/* rejectWithF as a building block (feature_tracker.cpp:731-736, the findFundamentalMat call), through the tracker's kernel: set b of n has the virtual-pixel pairs
 * pairs[4 first[b] .. 4 first[b + 1]) as ax ay bx by (a: previous frame, b: current), at most GF_REJECT_F_MAX_PAIRS of them, the threshold f_threshold[b] and
 * the seed seed[b], used as it is.  first, f_threshold, seed and results (may be NULL) are host tables; d_pairs and d_status are device memory.  d_status IS
 * WRITTEN: one byte per pair, 1 kept, 0 rejected.  One launch on `stream` (a hipStream_t, NULL = the null stream) whatever n; returns when it has run.  The call's job table is one
 * per process behind a lock held until the launch has run: calls from several threads or on several streams run one after another. */
int gf_reject_f_batch_device(int n, const int* first, const float* d_pairs, const double* f_threshold, const unsigned* seed, uint8_t* d_status, gf_reject_f_result* results,
                             void* stream);
/* The same on host memory (copy in, the launch, copy out; synchronous): for tests and callers without device memory */
int gf_reject_f_batch(int n, const int* first, const float* pairs, const double* f_threshold, const unsigned* seed, uint8_t* status, gf_reject_f_result* results);
/* The stage on PIXEL rows (feature_tracker.cpp:711-743 whole: the lift of :722-729 and the findFundamentalMat call), as the tracker launches it: set b has the
 * previous and current points prev_uv / cur_uv [2 first[b] .. 2 first[b + 1]) of a wh[2 b] x wh[2 b + 1] frame seen through cams[b] (any of the five models), a
 * threshold, a FOCAL_LENGTH (0: 460) and a seed, used as it is.  All tables are host memory; one launch, with every camera's lift inside the kernel.  _host:
 * the same through gfrf::reject and the shared lift on the host, no device needed; equal byte for byte for the models whose lift has no transcendental
 * (PINHOLE, MEI, PINHOLE_FULL, SCARAMUZZA), while a KANNALA_BRANDT set may differ in a borderline point. */
int gf_reject_f_pixels_batch(int n, const int* first, const gf_camera_model_ex* cams, const int* wh, const float* prev_uv, const float* cur_uv, const double* f_threshold,
                             const double* focal_length, const unsigned* seed, uint8_t* status, gf_reject_f_result* results);
int gf_reject_f_pixels_batch_host(int n, const int* first, const gf_camera_model_ex* cams, const int* wh, const float* prev_uv, const float* cur_uv, const double* f_threshold,
                                  const double* focal_length, const unsigned* seed, uint8_t* status, gf_reject_f_result* results);
/* F_threshold (F_THRESHOLD, parameters.cpp:201; feature_tracker.cpp:711-743) of a config file, and `reject_with_f`, a key of this repository's (absent or 0: off;
 * the reference has no switch of its own, its call is commented out) into out->f_threshold and out->enable; seed and focal_length are 0.  Refused by the
 * key's name: the switch on without a finite F_threshold > 0. */
int gf_reject_f_from_yaml(const char* config_file, gf_reject_f_cfg* out);
/* The same sets through gfrf::reject on the host, no device needed: the fallback (GF_REJECT_F_HOST=1) and the yardstick of the two calls above */
int gf_reject_f_batch_host(int n, const int* first, const float* pairs, const double* f_threshold, const unsigned* seed, uint8_t* status, gf_reject_f_result* results);
/* The track image: SHOW_TRACK and FeatureTracker::getTrackImage() (feature_tracker.cpp:849-905 drawTrack, :1047; what the node publishes as image_track) -- the
 * MONO8 frame trackImage tracked on (after the handle's colour / raw conversion and equalisation) as height x width x 3 bytes in the reference's channel order
 * (labelled bgr8 there), a dot per feature coloured (255 (1 - len), 0, 255 len) by len = min(1, track_cnt / 20), and a green arrow from each feature that LK
 * carried into the frame back to the point it was tracked from; a newly detected corner has none.  Geometry, colours, order (all dots in list order, then all
 * arrows) and rounding are the reference's; the outlines of OpenCV's thick circles and lines are replaced by exact integer distance tests, so boundary pixels of
 * a dot or stroke can differ from an OpenCV build and nothing else can ("Track image"; csrc/gf_track_draw.hpp).
 * gf_tracker_set_show_track: SHOW_TRACK of the `count` listed sequences (feature_tracker.cpp:304-305).  Off by default; a handle that never turns it on
 * allocates, copies, records and launches exactly what it did without these calls.  On: each frame the sequence takes leaves its list of primitives in host
 * memory, and the frame after the switch went on is already complete (the arrows need nothing from earlier frames).  The switch is a setting like the region
 * of interest: gf_tracker_reset_seq keeps it and drops the recorded picture; turning it off drops the picture too.  Refused as the lists of the track calls. */
int gf_tracker_set_show_track(gf_tracker* h, int count, const int* seq, int on);
/* getTrackImage (feature_tracker.cpp:1047; drawTrack :849-905) of each listed sequence into device memory.  `dst` IS WRITTEN, unlike every other gf_frame_ref
 * of this interface: dst[i] = the device pointer of the first byte of row 0 and the bytes from row to row (>= 3 x width, any alignment of both) of the image of
 * seq[i], e.g. an encoder's or a publisher's buffer, filled in place; exactly 3 x width bytes of each of the height rows are written.  The picture is that of
 * the moment the sequence's last track call returned, as in the reference: gf_tracker_set_prediction / gf_tracker_remove_outliers do not change it, and a
 * sequence that sat out the last calls gives its own last frame.  The background is read from the handle's own pyramid, never from the caller's frame.  One
 * launch for the list, ordered on the handle's stream; returns when the images are complete.  Refused with GF_ERR_INVALID, the message naming the list position,
 * and nothing written: a null handle or table, count < 0 or > batch, a sequence out of range or named twice, a sequence whose switch is off or that has no
 * frame recorded since the switch went on / gf_tracker_create / gf_tracker_reset_seq, a null data pointer, a pitch shorter than 3 x width. */
int gf_tracker_track_image_some_device(gf_tracker* h, int count, const int* seq, const gf_frame_ref* dst);
/* getTrackImage (feature_tracker.cpp:1047; drawTrack :849-905) of one sequence into host memory, rows `stride` bytes apart (>= 3 x width): the call above
 * through a staging image of the handle, obtained by the first call.  Refused as above. */
int gf_tracker_track_image(gf_tracker* h, int seq, uint8_t* dst, int stride);
/* drawTrack (feature_tracker.cpp:849-905) as a building block on host buffers (copies in, renders with the tracker's kernel, copies out; synchronous): `batch`
 * MONO8 frames of height rows, gray_pitch bytes apart (frame b at gray + b x height x gray_pitch), and for frame b n[b] <= cap features in row b of the
 * [batch][cap] tables cur_xy (x, y pairs), track_cnt, prev_xy and has_prev (feature i has an arrow back to prev_xy[i]; both may be NULL: no arrows) -> frame b at
 * dst + b x height x dst_pitch, dst_pitch >= 3 x width.  Any sizes and any alignment: the device copies take the host pointers' phase (address & 15).  `gray`
 * is read and `dst` read and written from the first byte to the last pixel of the last row -- (batch x height - 1) x pitch + one row of pixels, nothing behind
 * it -- so either may be a crop of a wider image; the bytes of `dst` in that span that are no pixel come back as they went.  Refused (GF_ERR_INVALID): track_cnt < 0, a point that is not finite or beyond
 * 2^20 in magnitude, short pitches, n[b] > cap.  GF_ERR_HIP if a byte next to the device copy of dst was written. */
int gf_draw_track_batch(const uint8_t* gray, size_t gray_pitch, int batch, int width, int height, const int* n, const float* cur_xy, const int* track_cnt,
                        const float* prev_xy, const uint8_t* has_prev, int cap, uint8_t* dst, size_t dst_pitch);
/* drawTrackbox's rectangles (feature_tracker.cpp:960-975; the boxes of trackImagebox, :374, whose filter is :565-599) over drawTrack's picture:
 * `cv::rectangle(imTrack, Rect(xmin, ymin, xmax - xmin, ymax - ymin), Scalar(0, 128, 255), 5)` after the arrows, as one frame primitive per box behind all dots
 * and strokes of the list.  In exact integers: nothing is drawn unless xmax > xmin && ymax > ymin; with X0 = xmin, X1 = xmax - 1, Y0 = ymin, Y1 = ymax - 1 a
 * pixel belongs to the frame iff X0 - 2 <= x <= X1 + 2 and Y0 - 2 <= y <= Y1 + 2 and not (X0 + 2 < x < X1 - 2 and Y0 + 2 < y < Y1 - 2); its bytes are
 * (0, 128, 255) whatever dots and strokes lie under it.  Only the rounded outer corners of OpenCV's thick rectangle can differ.  A tracker sequence with
 * show_track on and boxes in force records them with each frame, so gf_tracker_track_image* shows the boxes that frame was tracked under; drawTrackbox's yellow
 * dots for features inside a box (:982-987) have no counterpart, since no kept feature lies inside one.
 * gf_draw_track_boxes_batch: gf_draw_track_batch with, for frame b, the n_boxes[b] <= box_cap boxes of row b of the [batch][box_cap] table `boxes` (any int32_t
 * coordinates; clamped to +-2^20, which moves no pixel of an image). */
int gf_draw_track_boxes_batch(const uint8_t* gray, size_t gray_pitch, int batch, int width, int height, const int* n, const float* cur_xy, const int* track_cnt,
                              const float* prev_xy, const uint8_t* has_prev, int cap, uint8_t* dst, size_t dst_pitch, const int* n_boxes, const gf_box* boxes,
                              int box_cap);
/* FeatureTracker::removeOutliers (feature_tracker.cpp:1029-1045) */
int gf_tracker_remove_outliers(gf_tracker* h, int seq, const int* ids, int n);
/* public members ids / track_cnt / prev_pts (feature_tracker.h:85-88) */
int gf_tracker_get_state(gf_tracker* h, int seq, int* ids, int* track_cnt, float* prev_pts_xy, int cap, int* n);

int gf_tracker_set_profiling(gf_tracker* h, int enable); /* hipEvent timing of kernels (default off) */

/* Replaces `cv::createCLAHE(clip_limit, cv::Size(tiles_x, tiles_y))->apply(img, img)` on MONO8 frames (rosNodeTest.cpp:256-261, getImageFromMsg with EQUALIZE;
 * the reference calls it with the defaults, clip 40 and 8 x 8).  `batch` frames of height x width u8, back to back; d_src == d_dst is allowed.  Same bits as
 * OpenCV 4.2's scalar CV_8UC1 path (clahe.cpp), including the REFLECT_101 padding when the grid does not divide the frame; needs width > tiles_x and
 * height > tiles_y, clip_limit >= 0 (0: no clipping).  Asynchronous on `stream` (a hipStream_t, NULL = the null stream); device pointers of the current device. */
int gf_clahe_batch_device(const void* d_src, void* d_dst, int batch, int width, int height, double clip_limit, int tiles_x, int tiles_y, void* stream);
/* The same on host frames (copies in, equalises, copies out; synchronous): the building block the parity tests call.  src == dst is allowed. */
int gf_clahe_batch(const uint8_t* src, uint8_t* dst, int batch, int width, int height, double clip_limit, int tiles_x, int tiles_y);
/* Replaces `cv_bridge::toCvCopy(img_msg, sensor_msgs::image_encodings::MONO8)` of getImageFromMsg (rosNodeTest.cpp:238-254) on frames that are on the device:
 * `batch` frames of `height` rows, `src_pitch` bytes from row to row (>= width x bytes per pixel; frame b starts at d_src + b x height x src_pitch), `format` one
 * of GF_PIX_* -> `batch` tight height x width u8 frames at d_dst.  Colour: (R 4899 + G 9617 + B 1868 + 2^13) >> 14, alpha ignored (OpenCV 4.2 cvtColor);
 * GF_PIX_MONO8: a copy that removes the pitch; GF_PIX_BAYER_*: the bilinear demosaic fused with the same luma sum, border pixels equal to the nearest interior
 * pixel (cvtColor(COLOR_Bayer??2GRAY), generic loop; width and height >= 3); GF_PIX_YUV422_*: the luma byte of every pixel; GF_PIX_MONO16: (v + 128) / 257 on
 * little-endian pixels.  Any byte alignment of d_src, d_dst and src_pitch is accepted (rows whose bases, pitch and width are multiples of 4 move as whole
 * dwords).  d_src is never written; source and destination ranges that overlap are refused (GF_ERR_INVALID; GF_PIX_MONO8 alone may name the same tight frames
 * as both), as are an unknown format, src_pitch < width x bytes per pixel and sizes < 1.  Asynchronous on `stream` (a hipStream_t, NULL = the null stream);
 * device pointers of the current device. */
int gf_cvt_gray_batch_device(const void* d_src, size_t src_pitch, int format, void* d_dst, int batch, int width, int height, void* stream);
/* The same conversion (rosNodeTest.cpp:238-254) on host frames (copies in, converts, copies out; synchronous): the building block the parity tests call. */
int gf_cvt_gray_batch(const uint8_t* src, size_t src_pitch, int format, uint8_t* dst, int batch, int width, int height);
/* The same conversion (rosNodeTest.cpp:238-254) with a format of its own per frame, the building block of gf_tracker_set_seq_format: frame b lies at d_refs[b]
 * (device pointer of row 0, bytes from row to row >= width x bytes per pixel of its format) in d_formats[b] -> tight height x width u8 frame b at d_dst.  Both
 * tables are device-readable, [batch].  Each frame takes the load form its own pointer and pitch allow (any alignment) and gives the bytes
 * gf_cvt_gray_batch_device gives for it; nothing behind a ref is written.  Two launches at the most whatever the formats and the batch.  Asynchronous on
 * `stream`.  The host cannot read the tables: it refuses null pointers and sizes < 1 or beyond 2^31 - 1 pixels; an entry whose format is no GF_PIX_* writes
 * nothing for that frame and reads nothing, and an entry with a short pitch or a Bayer frame under 3 x 3 is the caller's error. */
int gf_cvt_gray_mixed_device(const gf_frame_ref* d_refs, const int* d_formats, void* d_dst, int batch, int width, int height, void* stream);
/* The same (rosNodeTest.cpp:238-254) on host buffers (copies in, converts, copies out; synchronous): src[b], pitch[b], format[b] per frame; the device copy
 * of a frame keeps its host pointer's phase (address & 15), so it takes the form it would take where it lies.  Refuses per frame, naming the frame, what
 * gf_cvt_gray_batch refuses: an unknown format, a pitch below a row, a Bayer frame under 3 x 3, a source that overlaps the destination. */
int gf_cvt_gray_mixed(const uint8_t* const* src, const size_t* pitch, const int* format, uint8_t* dst, int batch, int width, int height);
int gf_tracker_get_stats(gf_tracker* h, gf_tracker_stats* out);
int gf_tracker_reset_stats(gf_tracker* h);

/* ---- building blocks exposed for parity tests (device kernels on caller-provided HOST buffers) ---- */
/* cv::calcOpticalFlowPyrLK(prev,next,prevPts,nextPts,status,err,Size(21,21),maxLevel,
 *   TermCriteria(COUNT+EPS,30,0.01), useInitialFlow?OPTFLOW_USE_INITIAL_FLOW:0) as called at
 * feature_tracker.cpp:122,132,135,141.  pts are (x,y) float pairs. */
int gf_lk_track(const uint8_t* prev, const uint8_t* next, int width, int height, const float* prev_pts,
                float* next_pts, uint8_t* status, int n, int max_level, int use_initial_flow,
                long long* iterations);
/* The left-to-right matching of the stereo branch of FeatureTracker::trackImage (feature_tracker.cpp:259-303, kept there commented out), steps 2 and 3:
 *   cv::calcOpticalFlowPyrLK(cur_img, rightImg, cur_pts, cur_right_pts, status, err, cv::Size(21, 21), 3)                     (:273)
 * and, for a pair with FLOW_BACK,
 *   cv::calcOpticalFlowPyrLK(rightImg, cur_img, cur_right_pts, reverseLeftPts, statusRightLeft, err, cv::Size(21, 21), 3)     (:277)
 *   status[i] = status[i] && statusRightLeft[i] && inBorder(cur_right_pts[i]) && distance(cur_pts[i], reverseLeftPts[i]) <= 0.5   (:278-284)
 * with the default criteria (30 iterations / 0.01) and no initial flow in either direction; without FLOW_BACK the status is the forward pass's alone and a
 * right point may lie outside the image.  `count` pairs of tight width x height MONO8 frames, back to back in `left` and `right`; the points of pair b are
 * pts_xy[2 first[b] .. 2 first[b + 1]) (first[0] = 0, [count + 1] entries), flow_back[b] its switch.  right_xy, status and fwd_status (the forward pass alone;
 * may be null) are indexed like pts_xy.  One launch of the stereo kernel (stereo_lk_sized_kernel: one wavefront per point, lk_solve in both directions) for all
 * pairs; a pair's points reach it through both of its sources, rows of an LK table and a list of new corners.  Width a multiple of 4, both sizes >= 32
 * (gf_tracker_create's limits).  Synchronous.  The _device form takes the frames as device pointers on 4-byte boundaries; every other table is host memory. */
int gf_stereo_match_batch(const uint8_t* left, const uint8_t* right, int count, int width, int height, const int* first, const float* pts_xy,
                          const uint8_t* flow_back, float* right_xy, uint8_t* status, uint8_t* fwd_status);
int gf_stereo_match_batch_device(const void* d_left, const void* d_right, int count, int width, int height, const int* first, const float* pts_xy,
                                 const uint8_t* flow_back, float* right_xy, uint8_t* status, uint8_t* fwd_status);
/* cv::goodFeaturesToTrack(img, corners, max_corners, 0.01, min_dist, mask) as called at feature_tracker.cpp:198 */
int gf_good_features(const uint8_t* img, int width, int height, const uint8_t* mask, int max_corners,
                     int min_dist, float* corners_xy, int* n_out);
/* cornerMinEigenVal(img, eig, 3, 3) (inside goodFeaturesToTrack) */
int gf_min_eigen_val(const uint8_t* img, int width, int height, float* eig);
/* pyramid level l (0..3) of buildOpticalFlowPyramid and its Scharr derivative (interior only) */
int gf_pyramid_level(const uint8_t* img, int width, int height, int level, uint8_t* out, int16_t* deriv_xy);


/* profiling aid (no counterpart in the reference): kernels with a known byte count in the front end's access patterns, to calibrate rocprofv3's
 * FETCH_SIZE (scripts/pmc_collect.sh).  mode 0 streaming 16 B/lane, 1 LK 32x32 tile refill with 64-byte-aligned row segments, 2 the same straddling
 * two 64-byte lines.  Outputs: bytes the lanes requested, distinct 64-byte lines touched, kernel time. */
int gf_calib_fetch(int mode, size_t buffer_bytes, double* requested_bytes, double* lines64, double* ms);


/* ------------------------------------------------------------------ back end: Estimator::optimization() */
/* Replaces the Ceres problem built and solved in Estimator::optimization() (vins_estimator/src/estimator/estimator.cpp:2890-3327:
 * vector2double -> ceres::Solve(DENSE_SCHUR, DOGLEG, max_num_iterations) ) and the construction of the next marginalisation prior
 * (estimator.cpp:3334-3631, factor/marginalization_factor.cpp:119-308).  A window is handed over exactly as the reference hands it to
 * Ceres: the para_* arrays of vector2double (estimator.cpp:2276-2353) plus the constructor arguments of each factor. */
typedef struct gf_ba gf_ba;

/* parameter-block ids used by priors: kind * 4096 + index */
enum { GF_POSE = 0, GF_SPEEDBIAS = 1, GF_EX_POSE = 2, GF_EX_WHEEL = 3, GF_SX = 4, GF_SY = 5, GF_SW = 6, GF_TD = 7, GF_TD_WHEEL = 8, GF_FEATURE = 9,
       GF_RCV_DT = 10, GF_RCV_DDT = 11, GF_YAW = 12, GF_ANC = 13 };

typedef struct gf_ba_cfg {
    int window_size;   /* WINDOW_SIZE (parameters.h:24 fixes 10; here a runtime value) */
    int max_features;  /* capacity of para_Feature (NUM_OF_F, parameters.h:25) */
    int max_visual;    /* capacity of visual factors per window */
    int batch;         /* independent windows solved per call */
    int max_gnss;      /* capacity of GnssPsrDoppFactor per window; 0 builds the handle without the GNSS blocks (gnss_enable: 0) */
} gf_ba_cfg;

typedef struct gf_ba_window {
    int W, n_feature, n_visual, n_imu, n_wheel;
    /* SetParameterBlockConstant decisions of estimator.cpp:2990-3100, :3233-3246 */
    int fix_ex_pose, fix_ex_wheel, fix_ix, fix_td, fix_td_wheel, fix_poses;
    double G[3];              /* gravity, estimator.h `g` */
    double vis_sqrt_info;     /* FOCAL_LENGTH / 1.5 (estimator.cpp:193) */
    /* parameter blocks, in/out (estimator.h:335-341) */
    double* para_Pose;        /* (W+1) x 7: px py pz qx qy qz qw */
    double* para_SpeedBias;   /* (W+1) x 9 */
    double* para_Ex_Pose;     /* 7 */
    double* para_Ex_Pose_wheel; /* 7 */
    double* para_Ix;          /* sx, sy, sw */
    double* para_Td;          /* 1 */
    double* para_Td_wheel;    /* 1 */
    double* para_Feature;     /* n_feature inverse depths */
    const unsigned char* feature_fixed; /* estimate_flag == 1 -> constant (estimator.cpp:3291-3292) */
    /* ProjectionTwoFrameOneCamFactor(pts_i, pts_j, velocity_i, velocity_j, td_i, td_j) on (Pose[i], Pose[j], Ex_Pose, Feature[f], Td) */
    /* preconditions, checked at upload (GF_ERR_INVALID): i < j; all factors of a feature name the same start frame i and bring the same start-frame observation;
       a feature has at most one factor per frame j -- what estimator.cpp:3269-3297 builds (one factor per later observation, all from feature_per_frame[0]) */
    const int* vis_feature; const int* vis_i; const int* vis_j;
    const double* vis_pts_i; const double* vis_pts_j; const double* vis_vel_i; const double* vis_vel_j; const double* vis_td_i; const double* vis_td_j;
    /* IMUFactor(pre_integrations[i+1]) on (Pose[i], SpeedBias[i], Pose[i+1], SpeedBias[i+1]); delta_q as (w,x,y,z); 15x15 row-major */
    const int* imu_i; const double* imu_sum_dt; const double* imu_delta_p; const double* imu_delta_q; const double* imu_delta_v;
    const double* imu_lin_ba; const double* imu_lin_bg; const double* imu_jacobian; const double* imu_covariance;
    /* WheelFactor(pre_integrations_wheel[i+1]); jacobian 6x3, covariance 6x6 row-major; wh_lin = linearized sx, sy, sw, td */
    const int* wh_i; const double* wh_sum_dt; const double* wh_delta_p; const double* wh_delta_q; const double* wh_jacobian;
    const double* wh_covariance; const double* wh_lin; const double* wh_lin_vel; const double* wh_lin_gyr; const double* wh_vel_1; const double* wh_gyr_1;
    /* MarginalizationFactor(last_marginalization_info): linearized_jacobians (n x n row-major), linearized_residuals, keep_block_data */
    int prior_n, prior_nblocks;
    const int* prior_block_id; const double* prior_J; const double* prior_r; const double* prior_x0;
    /* GNSS (estimator.cpp:2904-2941, :3178-3229, :3390-3431): blocks and factors.  gnss_enabled = gnss_ready; the factors enter the solve
     * unless gnss_lowspeed (estimator.cpp:3178), and enter the MARGIN_OLD marginalisation whenever gnss_enabled (:3390).
     * gnss_data per factor (16 doubles): sv_pos 3, sv_vel 3, svdt, svddt, tgd, pr_uura, dp_uura, psr, dopp, wavelength, time of GPS week [s], 0.
     * What GnssPsrDoppFactor's constructor derives from observation + ephemeris (gnss_psr_dopp_factor.cpp:3-47) is handed over precomputed. */
    int gnss_enabled, gnss_lowspeed, n_gnss, has_anchor;
    double* para_rcv_dt;         /* 4 (W+1), in/out */
    double* para_rcv_ddt;        /* (W+1) */
    double* para_yaw_enu_local;  /* 1 (held constant, estimator.cpp:2932) */
    double* para_anc_ecef;       /* 3 */
    double gnss_ddt_weight;      /* GNSS_DDT_WEIGHT, parameters.cpp:549 */
    double anchor_value[7];      /* PoseAnchorFactor on Pose[0] (estimator.cpp:2943-2951), sqrt_info 120 */
    const double* gnss_iono;     /* 8 Klobuchar parameters */
    const int* gnss_frame;       /* i: the factor uses rcv_dt[4 i + sys] and rcv_ddt[i] */
    const int* gnss_lower;       /* lower_idx: the factor sits on (Pose, SpeedBias)[lower_idx] and [lower_idx + 1] */
    const int* gnss_sys;         /* sys_idx 0..3 */
    const double* gnss_ratio;    /* ts_ratio */
    const double* gnss_data;     /* n_gnss x 16 */
    const double* gnss_headers;  /* Headers[0..W]: DtDdtFactor(Headers[i+1] - Headers[i]), estimator.cpp:3214-3223 */
    /* PoseSubsetParameterization (pose_subset_parameterization.cpp:10-56) of the camera / wheel extrinsic, estimator.cpp:2969-2985, :3010-3026:
     * bit q (0-2 translation, 3-5 rotation) set = component q of the block's increment is zeroed in Plus.  The block keeps its six columns and the
     * solver its full step (ComputeJacobian stays the identity: the reference's quirk); only the candidate point is masked.  0 = ADJUST_*_ALL.
     * Use gf_pose_subset_mask(extrinsic_type) for the YAML values. */
    int ex_pose_mask, ex_wheel_mask;
} gf_ba_window;

/* `extrinsic_type` / `extrinsic_type_wheel` of the YAML files (parameters.cpp:280-306, :394-420) -> constancy mask: 0 ALL {}, 1 TRANSLATION {3,4,5},
 * 2 ROTATION {0,1,2}, 3 NO_Z {2}, 4 NO_ROTATION_NO_Z {2,3,4,5}; any other value leaves the reference's zero-initialised enum = *_TRANSLATION. */
int gf_pose_subset_mask(int extrinsic_type);

typedef struct gf_ba_summary {
    int iterations, successful_steps, termination; /* 0 max iterations, 1 function tol, 2 parameter tol, 3 gradient tol, 4 failure */
    double initial_cost, final_cost, radius;
} gf_ba_summary;

/* caller-owned output of gf_ba_marginalize: J is n x n (row-major, capacity cap_n*cap_n), block ids already address-shifted */
typedef struct gf_ba_prior {
    int cap_n, cap_blocks;
    int n, nblocks, m, valid;
    int* block_id; double* J; double* r; double* x0;
} gf_ba_prior;

typedef struct gf_ba_stats {
    double ms_upload, ms_solve, ms_marginalize, ms_download;   /* hipEvent times accumulated over calls */
    double ms_jtj;                                             /* time inside the visual J^T J (MFMA) kernel */
    long long solves, jtj_launches, jtj_flops;                 /* jtj_flops: MFMA flops issued by that kernel */
    double ms_step;                                            /* time inside ba_step (one full dogleg step per solve is timed) */
    long long step_launches, step_flops;                       /* step_flops: Schur SYRK + Cholesky + substitutions of the timed launches */
    long long jtj_alg_flops;                                   /* algorithmic flops of the timed visual J^T J launches: Nv * 2 * 2 * 91 per window */
    double ms_jtj_contract;                                    /* split formulation (gf_ba_set_split_jtj): time inside the contraction-only MFMA kernel */
    long long jtj_contract_launches;
} gf_ba_stats;

int gf_ba_create(const gf_ba_cfg* cfg, gf_ba** out);
/* north_star's formulation of the visual sweep as a measured alternative (fixed camera extrinsic only): "residual/Jacobian sweep ... writing block-rows that an MFMA
 * J^T J contraction ... reduce[s]" -- the sweep stores every factor's 2 x 16 block row in HBM, a second kernel does nothing but contract them on the matrix cores.
 * Same bits as the fused kernel (same products, same order).  Off by default: it costs a 256-byte round trip per factor. */
int gf_ba_set_split_jtj(gf_ba* h, int on);
int gf_ba_destroy(gf_ba* h);
/* ceres::Solve on `count` <= batch windows (estimator.cpp:3303-3318 with max_solver_time disabled); states updated in place */
int gf_ba_solve(gf_ba* h, gf_ba_window* windows, int count, int max_iters, gf_ba_summary* summaries);
/* next prior; mode 0 = MARGIN_OLD (estimator.cpp:3334-3534), 1 = MARGIN_SECOND_NEW (:3536-3631) */
int gf_ba_marginalize(gf_ba* h, const gf_ba_window* windows, int count, int mode, gf_ba_prior* priors);
/* the same on windows that the preceding gf_ba_solve / gf_ba_upload left resident: only the parameter blocks (changed by double2vector's gauge fix,
 * estimator.cpp:3327-3337) are uploaded again, only the priors' n x n blocks come back.  slots[i]: position of windows[i] in the resident batch */
int gf_ba_marginalize_resident(gf_ba* h, const int* slots, const gf_ba_window* windows, int n, int mode, gf_ba_prior* priors);
/* priors == NULL above: the priors stay in the handle's host mirrors and every owner fetches its own (callable concurrently for different slots) */
int gf_ba_unpack_prior_slot(gf_ba* h, int slot, int mode, gf_ba_prior* prior);
/* throughput path: windows stay resident in HBM between calls */
int gf_ba_upload(gf_ba* h, const gf_ba_window* windows, int count);
int gf_ba_solve_resident(gf_ba* h, int max_iters, int marginalize_mode /* -1: none */, int reset_state);
/* same, returning as soon as the work is enqueued (the reference runs processImage on its own thread, estimator.cpp:209); gf_ba_wait joins */
int gf_ba_solve_resident_async(gf_ba* h, int max_iters, int marginalize_mode, int reset_state);
int gf_ba_wait(gf_ba* h);
int gf_ba_download(gf_ba* h, gf_ba_window* windows, int count, gf_ba_summary* summaries, gf_ba_prior* priors);
/* the newest pose (para_Pose[W]: px py pz qx qy qz qw) of the first `count` resident windows into a DEVICE array [count][7] -- the payload of the
 * per-step pose gather across GPUs (north_star; there is no counterpart in the single-process reference).  Enqueued behind a pending
 * asynchronous solve (complete after gf_ba_wait); otherwise complete on return. */
int gf_ba_export_newest_poses(gf_ba* h, void* d_out, int count);
/* The same solve for callers that own many windows on many threads (gf_estimator_group_*; no counterpart in the reference, whose Estimator owns one
 * window): gf_ba_pack_slot packs one window into slot `slot` of the handle's staging tables -- callable concurrently for different slots, one thread per
 * slot --, gf_ba_solve_packed closes the batch (upload, ceres::Solve on the listed slots -- slots not listed sit this batch out --, one download of all
 * states) and gf_ba_unpack_slot copies the solved state and the summary of a slot back into its owner's window (again callable concurrently for
 * different slots).  Results are identical to gf_ba_solve on the same windows.  gf_ba_marginalize_resident then takes the same slot numbers. */
/* Device-resident priors: a prior fetched with gf_ba_unpack_prior_slot(..., prior->J == NULL) leaves its n x n factor on the device; the slot's next window says
 * so with prior_n > 0 and prior_J == NULL (block ids, r and x0 as usual) and the solve copies it device to device -- 60 KB per window and frame that cross the
 * bus in neither direction.  gf_ba_fetch_resident_prior reads it back for whoever wants to look at it. */
int gf_ba_pack_slot(gf_ba* h, int slot, const gf_ba_window* window);
int gf_ba_fetch_resident_prior(gf_ba* h, int slot, int n, double* J);
int gf_ba_solve_packed(gf_ba* h, const int* slots, int n, int max_iters);
int gf_ba_unpack_slot(gf_ba* h, int slot, gf_ba_window* window, gf_ba_summary* summary);
/* ceres::Solver::Options::max_solver_time_in_seconds (estimator.cpp:3312-3315) for the following gf_ba_solve / gf_ba_solve_resident calls; 0 (default) = not
 * honoured: the iterations are enqueued back to back.  With a limit the host synchronises before every iteration, as Ceres checks its clock there. */
int gf_ba_set_max_solver_time(gf_ba* h, double seconds);
int gf_ba_get_stats(gf_ba* h, gf_ba_stats* out);
int gf_ba_debug_stamps(gf_ba* h, long long* out, int n); /* per-phase clock stamps of ba_step (profiling builds, -DGF_PROFILE_STEP) */
int gf_ba_reset_stats(gf_ba* h);
/* inspection for parity tests: H = J^T J, g = J^T r (loss-corrected, unscaled), cost; canonical column order
 * [free blocks: pose0, sb0, pose1, ..., ex, exw, sx, sy, sw, td, tdw | free features by index] */
int gf_ba_linearize(gf_ba* h, const gf_ba_window* w, int cap, double* H, double* g, double* cost, int* n_f, int* n_e, int* col_block_id);

/* Estimator::double2vector, pose part (estimator.cpp:2440-2497, USE_IMU branch; R2ypr/ypr2R in degrees, utility.h:78-118):
 * R0_before = Rs[0] (3x3 row-major) and P0_before = Ps[0] before the solve; outputs Rs (W+1)x9 row-major, Ps/Vs/Bas/Bgs (W+1)x3. */
int gf_ba_double2vector(int W, const double* R0_before, const double* P0_before, const double* para_Pose, const double* para_SpeedBias,
                        double* Rs, double* Ps, double* Vs, double* Bas, double* Bgs);

/* IntegrationBase::push_back loop (factor/integration_base.h:39-167), host side; noise = ACC_N, GYR_N, ACC_W, GYR_W */
int gf_imu_preintegrate(int n, const double* dt, const double* acc, const double* gyr, const double* acc0, const double* gyr0, const double* ba,
                        const double* bg, const double* noise, double* delta_p, double* delta_q, double* delta_v, double* jacobian,
                        double* covariance, double* sum_dt);
/* The 3-vector / quaternion part of the same loop alone (round 6): delta_p, delta_q (w x y z), delta_v, sum_dt -- bit for bit what gf_imu_preintegrate returns for them,
 * without the Jacobian and the covariance (99 % of the arithmetic).  Estimator::checkimu (estimator.cpp:2173-2216) reads delta_v / sum_dt of every frame on every image. */
int gf_imu_preintegrate_state(int n, const double* dt, const double* acc, const double* gyr, const double* acc0, const double* gyr0, const double* ba,
                              const double* bg, double* delta_p, double* delta_q, double* delta_v, double* sum_dt);
/* The same loop for many intervals at once ON THE DEVICE (row B2 batched): interval i owns the samples first[i] .. first[i+1]-1 of dt / acc / gyr
 * and row i of acc0 / gyr0 / ba / bg (n x 3) and of the outputs (delta_p n x 3, delta_q n x 4 as w x y z, delta_v n x 3, jacobian / covariance n x 225, sum_dt n).
 * One wavefront per interval; every result is bit-identical to gf_imu_preintegrate on the same samples.  No CPU fallback: GF_ERR_NO_DEVICE without a GPU. */
typedef struct gf_preint gf_preint;
int gf_preint_create(gf_preint** out);
int gf_preint_destroy(gf_preint* h);
int gf_imu_preintegrate_batch(gf_preint* h, int n, const int* first, const double* dt, const double* acc, const double* gyr, const double* acc0, const double* gyr0,
                              const double* ba, const double* bg, const double* noise, double* delta_p, double* delta_q, double* delta_v, double* jacobian,
                              double* covariance, double* sum_dt);
int gf_preint_stats(gf_preint* h, long long* launches, long long* intervals, double* kernel_ms); /* kernel_ms: hipEvent time of the kernel alone, summed */
/* The per-feature sweeps of the measurement side for many windows at once ON THE DEVICE, one thread per feature, decisions and depths
 * bit-identical to the host loops of the estimator:
 *   gf_triangulate_with_depth_batch  FeatureManager::triangulateWithDepth, feature_manager.cpp:726-799 (estimated_depth / estimate_flag updated in place)
 *   gf_moving_consistency_batch      Estimator::movingConsistencyCheckW, estimator.cpp:3955-3995 (remove[f] = 1 for the ids the reference puts into removeIndex)
 * Window b: Rs / Ps ((W+1) x 9 row-major / (W+1) x 3), tic (3), ric (9), features first_feature[b] .. first_feature[b+1]-1 (feature_manager's list order);
 * feature f: start_frame[f], observations first_obs[f] .. first_obs[f+1]-1, each x, y, z of the normalised point and the depth-camera depth.
 * The _each forms take depth_threshold / init_depth / focal_length as arrays of B values, one per window, for windows of estimators that differ in them
 * (gf_estimator_group_create_each); with equal values they leave the bits of the scalar forms. */
typedef struct gf_featsweep gf_featsweep;
int gf_featsweep_create(gf_featsweep** out);
int gf_featsweep_destroy(gf_featsweep* h);
int gf_triangulate_with_depth_batch(gf_featsweep* h, int B, int W, const double* Rs, const double* Ps, const double* tic, const double* ric, const int* first_feature,
                                    const int* start_frame, const int* first_obs, const double* obs, double depth_threshold, double init_depth,
                                    double* estimated_depth, int* estimate_flag);
int gf_moving_consistency_batch(gf_featsweep* h, int B, int W, const double* Rs, const double* Ps, const double* tic, const double* ric, const int* first_feature,
                                const int* start_frame, const int* first_obs, const double* obs, const double* estimated_depth, double focal_length, int* remove);
int gf_triangulate_with_depth_batch_each(gf_featsweep* h, int B, int W, const double* Rs, const double* Ps, const double* tic, const double* ric, const int* first_feature,
                                         const int* start_frame, const int* first_obs, const double* obs, const double* depth_threshold, const double* init_depth,
                                         double* estimated_depth, int* estimate_flag);
int gf_moving_consistency_batch_each(gf_featsweep* h, int B, int W, const double* Rs, const double* Ps, const double* tic, const double* ric, const int* first_feature,
                                     const int* start_frame, const int* first_obs, const double* obs, const double* estimated_depth, const double* focal_length, int* remove);
int gf_featsweep_stats(gf_featsweep* h, long long* launches, long long* features, double* kernel_ms);
/* WheelIntegrationBase::push_back loop (factor/wheel_integration_base.h:41-178); noise = VEL_N_wheel, GYR_N_wheel; lin = sx, sy, sw */
int gf_wheel_preintegrate(int n, const double* dt, const double* vel, const double* gyr, const double* vel0, const double* gyr0, const double* lin,
                          const double* noise, double* delta_p, double* delta_q, double* jacobian, double* covariance, double* sum_dt);

/* ------------------------------------------------------------------------------------------------------------------------------
 * Estimator: the call surface of Estimator::processImage and its bookkeeping, one handle per
 * sequence.  Replaces, in vins_estimator/src/estimator/estimator.h: inputIMU :104, inputWheel :106, inputFeature :108,
 * inputImage :105, processImage :110 (via processMeasurements :113), and the FeatureManager it owns (feature_manager.h:139-215).
 * The dense work (Estimator::optimization, estimator.cpp:2890-3636) runs on the HIP back end behind gf_ba_*.
 * Built: RGB-D + IMU (+ wheel) (+ GNSS) configuration, stationary / wheel-activated initialisation (estimator.cpp:1557-1682) and the SfM branch behind
 * them for recordings that begin in motion (estimator.cpp:1684-1926; relativePoseWithDepth, GlobalSFM::constructWithDepth, visualInitialAlign),
 * MULTIPLE_THREAD 0/1 data flow (processed synchronously); GNSS: measurement gating, clock / anchor / yaw states, factors in the solve and the
 * marginalisation, GNSSVIAlign with its initialiser, broadcast ephemerides -> satellite states (gf_estimator_input_ephem + gf_estimator_input_gnss_raw;
 * or states handed in, gf_gnss_obs).  Not built: monocular (DEPTH 0) initialisation, line / plane / motion factors.
 * ------------------------------------------------------------------------------------------------------------------------------ */
typedef struct gf_estimator gf_estimator;

typedef struct gf_estimator_cfg {
    int window_size;        /* WINDOW_SIZE, parameters.h:24 */
    int max_features;       /* NUM_OF_F, parameters.h:25 */
    int max_visual;         /* capacity of visual factors per window */
    int use_imu, use_wheel, depth;                              /* imu / wheel / depth, parameters.cpp:160-176 */
    int estimate_extrinsic, estimate_wheel_extrinsic, estimate_wheel_intrinsic, estimate_td, estimate_td_wheel;
    int use_mcc, wdetect, stationary_detect, only_initial_with_wheel, multiple_thread;
    int num_iterations;     /* max_num_iterations */
    int with_tracker;       /* own a FeatureTracker (gf_estimator_input_image); `tracker` below configures it */
    double acc_n, gyr_n, acc_w, gyr_w, g_norm, wheel_vel_n, wheel_gyr_n;
    double min_parallax_px; /* keyframe_parallax (pixels at FOCAL_LENGTH) */
    double depth_threshold, init_depth, focal_length; /* depth_threshold; INIT_DEPTH parameters.cpp:478; FOCAL_LENGTH parameters.h:23 */
    double td, td_wheel, sx, sy, sw;
    double tic[3], ric[9], tio[3], rio[9];  /* body_T_cam0, body_T_wheel (row-major rotations) */
    gf_tracker_cfg tracker;
    /* GNSS (parameters.cpp:519-552): gnss_enable; thresholds of processGNSS (estimator.cpp:1497-1523); GNSS_DDT_WEIGHT = 1 / gnss_ddt_sigma;
     * max_gnss_per_frame: capacity of gnss_meas_buf[i]; gnss_iono[8]: gnss_iono_default_parameters */
    int gnss_enable, gnss_track_num_thres, max_gnss_per_frame;
    double gnss_elevation_thres, gnss_psr_std_thres, gnss_dopp_std_thres, gnss_ddt_sigma, gnss_local_time_diff;
    double gnss_iono[8];
    /* SOLVER_TIME (`max_solver_time`, parameters.cpp:343): the solve gets 4/5 of it when the oldest frame will be marginalised, all of it otherwise
     * (estimator.cpp:3312-3315).  0 = not honoured (parity runs: the oracle counts iterations only).  A wall-clock cut makes the members of one
     * batch end after different iteration counts depending on who shares the batch, so gf_estimator_group_create refuses a value > 0. */
    double max_solver_time;
    /* extrinsic_type / extrinsic_type_wheel (parameters.cpp:394-420, :280-306): which components of the camera / wheel extrinsic the solver may move
     * once the block is free (estimate_extrinsic / estimate_wheel_extrinsic): 0 all, 1 translation, 2 rotation, 3 no z, 4 no rotation and no z */
    int extrinsic_type, extrinsic_type_wheel;
} gf_estimator_cfg;

/* One L1 observation of a GNSS epoch as Estimator::inputGNSS receives it (ObsPtr), together with what GnssPsrDoppFactor's constructor derives from
 * the matching ephemeris (gnss_psr_dopp_factor.cpp:3-47 via gnss_comm eph2pos / geph2pos / eph2svdt: not part of this build):
 * the satellite state at transmission time. */
typedef struct gf_gnss_obs {
    int sat;                 /* satellite number (tracking statistics, estimator.cpp:1497-1511) */
    int sys;                 /* constellation index 0 GPS, 1 GLO, 2 GAL, 3 BDS (gnss_comm::sys2idx); < 0: any other system, dropped (estimator.cpp:1463-1465) */
    double time;             /* time2sec(obs->time) [s] */
    double psr, dopp, psr_std, dopp_std, wavelength;   /* L1 pseudorange [m], Doppler [Hz], their standard deviations, carrier wavelength [m] */
    double sv_pos[3], sv_vel[3], svdt, svddt, tgd, pr_uura, dp_uura, tow;
} gf_gnss_obs;

int gf_estimator_default_cfg(gf_estimator_cfg* cfg);   /* values of config/realsense/m2dgrp.yaml */
int gf_estimator_create(const gf_estimator_cfg* cfg, gf_estimator** out);
int gf_estimator_destroy(gf_estimator* h);
int gf_estimator_input_imu(gf_estimator* h, double t, const double* acc, const double* gyr);
int gf_estimator_input_wheel(gf_estimator* h, double t, const double* vel, const double* gyr);
/* Broadcast ephemerides as Estimator::inputEphem receives them (estimator.h:97, estimator.cpp:1428-1437; gnss_comm::Ephem / GloEphem) and the L1 entry of an
 * observation (gnss_comm::Obs).  gtime_t fields are seconds (time2sec).  With these the library derives the satellite state itself, the way
 * GnssPsrDoppFactor's constructor does (gnss_psr_dopp_factor.cpp:3-47: transmission time, eph2svdt / eph2pos / eph2vel or their GLONASS counterparts);
 * gnss_comm is not vendored by the reference, so eph2pos etc. are restated from the published broadcast-orbit algorithms (IS-GPS-200 Kepler model, BeiDou
 * GEO rotation, GLONASS ICD Runge-Kutta with 60 s steps; velocities and clock drifts by the 1 ms difference quotient RTKLIB uses). */
typedef struct gf_gnss_ephem {
    int sat, sys, prn;       /* satellite number, constellation index (0 GPS, 2 GAL, 3 BDS), PRN within it (BeiDou GEO: prn <= 5 or >= 59) */
    double toe, toc, toe_tow; /* time2sec(toe), time2sec(toc), toe as seconds of the constellation's week */
    double A, e, i0, OMG0, omg, M0, delta_n, OMG_dot, i_dot, cuc, cus, crc, crs, cic, cis, af0, af1, af2, tgd0, ura;
} gf_gnss_ephem;
typedef struct gf_gnss_glo_ephem {
    int sat;
    double toe;              /* time2sec(toe) */
    double pos[3], vel[3], acc[3], tau_n, gamma;   /* PZ-90 state at toe [m, m/s, m/s^2], clock bias [s] and relative frequency bias */
} gf_gnss_glo_ephem;
typedef struct gf_gnss_raw_obs {
    int sat, sys;            /* as in gf_gnss_obs; sys 1 = GLONASS */
    double time, psr, dopp, psr_std, dopp_std, freq, tow;   /* reception time [s], L1 pseudorange [m], Doppler [Hz], their deviations, carrier frequency [Hz], time of week */
} gf_gnss_raw_obs;
/* the satellite state of one observation from its ephemeris (exactly one of eph / geph non-NULL): what gf_estimator_input_gnss_raw does per observation */
int gf_gnss_obs_from_ephem(const gf_gnss_raw_obs* raw, const gf_gnss_ephem* eph, const gf_gnss_glo_ephem* geph, gf_gnss_obs* out);
/* satellite position [m] and clock bias [s] at time t (eph2pos / geph2pos): building block entry for tests */
int gf_gnss_eph2pos(double t, const gf_gnss_ephem* eph, const gf_gnss_glo_ephem* geph, double* pos3, double* svdt);

/* Estimator::inputGNSS (estimator.h:99, estimator.cpp:397): one epoch; inputGNSSTimeDiff (estimator.cpp:1450); inputIonoParams (estimator.h:98) */
int gf_estimator_input_gnss(gf_estimator* h, double t, const gf_gnss_obs* obs, int n);
/* the same with raw observations: processGNSS then picks, per observation, the ephemeris of its satellite nearest in toe within EPH_VALID_SECONDS (7200 s)
 * (estimator.cpp:1467-1495; observations without one are skipped), evaluates the elevation gate at the reception time and derives the satellite state */
int gf_estimator_input_gnss_raw(gf_estimator* h, double t, const gf_gnss_raw_obs* obs, int n);
int gf_estimator_input_ephem(gf_estimator* h, const gf_gnss_ephem* eph);            /* Estimator::inputEphem, estimator.cpp:1428-1437 */
int gf_estimator_input_glo_ephem(gf_estimator* h, const gf_gnss_glo_ephem* geph);
int gf_estimator_input_gnss_time_diff(gf_estimator* h, double diff_t_gnss_local);
int gf_estimator_input_iono_params(gf_estimator* h, const double* params8);
/* GNSSVIAlign (estimator.cpp:1928-2043) runs inside the library: GNSSVIInitializer (initial/gnss_vi_initializer.cpp: coarse SPP localisation of the
 * window's measurements, yaw alignment on the Doppler residuals, anchor refinement) on the satellite states of gf_gnss_obs, under the reference's
 * preconditions (visual-inertial part initialised, mean horizontal speed of the window >= 0.3 m/s).  A caller that has its own fix may hand it in
 * instead: the next alignment attempt then takes refined_xyzt = anc_ecef + rcv_dt[4], yaw and clock drift from here (rcv_dt[k] = 0: system k unobserved). */
int gf_estimator_set_gnss_alignment(gf_estimator* h, const double* anc_ecef, double yaw_enu_local, const double* rcv_dt4, double rcv_ddt);
/* gnss[8]: gnss_ready, lowspeed, #valid measurements of the newest frame, first_optimization, then 4 reserved; any pointer may be NULL.
 * rcv_dt 4 (W+1), rcv_ddt (W+1), anc_ecef 3, ecef_pos 3, enu_pos 3 (updateGNSSStatistics, estimator.cpp:2045-2058) */
int gf_estimator_get_gnss_state(gf_estimator* h, int* gnss, double* rcv_dt, double* rcv_ddt, double* yaw_enu_local, double* anc_ecef, double* ecef_pos, double* enu_pos);
/* inputFeature + processMeasurements: one call = one processImage once IMU / wheel data cover the frame time */
int gf_estimator_input_feature(gf_estimator* h, double t, const gf_feature_obs* obs, int n);
/* Estimator::processImage(image, header) (estimator.h:110, estimator.cpp:843-1163) called directly, as the reference's public method allows: the frame
 * goes through the keyframe vote, initialisation / optimisation and the window shift with whatever processIMU / processWheel have integrated so far
 * (inputFeature does this for the frames it takes off the queue).  Needs at least one processed IMU sample when use_imu is set. */
int gf_estimator_process_image(gf_estimator* h, double header, const gf_feature_obs* obs, int n);
/* inputImage: trackImage on the owned tracker, then inputFeature (every second frame when multiple_thread, estimator.cpp:226).  The frame is in the format of
 * cfg.tracker.pixel_format (gf_estimator_default_cfg: GF_PIX_MONO8; no YAML key, the reference has none): with a colour or raw format `gray` holds pixels of that format and
 * `stride` >= width x bytes per pixel, and the tracker converts on the device what the node's getImageFromMsg converts on the host (rosNodeTest.cpp:238-254) */
int gf_estimator_input_image(gf_estimator* h, double t, const uint8_t* gray, int stride, const uint16_t* depth, int dstride,
                             gf_feature_obs* out, int cap, int* n_out);
/* window state; arrays of (window_size+1) entries, any pointer may be NULL.  info[16]: frame_count, solver_flag, marginalization_flag,
 * #features, prior valid, prior n, systemstationary, last iterations, last successful steps, #optimizations, openExWheelEstimation,
 * last_track_num, long_track_num, new_feature_num, sum_of_back, sum_of_front.  extr[32]: tic 3, ric 9, tio 3, rio 9, sx, sy, sw, td,
 * td_wheel, last initial cost, last final cost, last_average_parallax */
int gf_estimator_get_state(gf_estimator* h, double* Ps, double* Rs, double* Vs, double* Bas, double* Bgs, double* Headers, int* info, double* extr);
/* The region of interest of an estimator that owns its tracker (cfg.with_tracker): gf_tracker_set_roi on that tracker's one sequence -- mask = height x width
 * bytes of the tracker's frame size, rows `stride` bytes apart, non-zero = allowed, NULL clears; it holds from the next gf_estimator_input_image on.
 * GF_ERR_INVALID without a tracker, and as gf_tracker_set_roi refuses. */
int gf_estimator_set_roi(gf_estimator* h, const uint8_t* mask, int stride);
/* The exclusion boxes of an estimator that owns its tracker: gf_tracker_set_boxes_some on that tracker's one sequence (trackImagebox's boxes,
 * feature_tracker.cpp:374, :565-599, :960-975), in force from the next gf_estimator_input_image until replaced; n == 0 clears.  GF_ERR_INVALID without a
 * tracker, and as gf_tracker_set_boxes_some refuses. */
int gf_estimator_set_boxes(gf_estimator* h, const gf_box* boxes, int n);
/* SHOW_TRACK and getTrackImage (feature_tracker.cpp:849-905, :1047) of an estimator that owns its tracker: gf_tracker_set_show_track / gf_tracker_track_image
 * on that tracker's one sequence -- the picture of the last gf_estimator_input_image, height x width x 3 bytes, rows `stride` bytes apart.  GF_ERR_INVALID
 * without a tracker, and as those calls refuse. */
int gf_estimator_set_show_track(gf_estimator* h, int on);
int gf_estimator_get_track_image(gf_estimator* h, uint8_t* dst, int stride);
/* rejectWithF (feature_tracker.cpp:711-743) of an estimator that owns its tracker: gf_tracker_set_seq_reject_f on its one sequence, from the next
 * gf_estimator_input_image on; NULL turns it off.  Refused for an estimator created without a tracker. */
int gf_estimator_set_reject_f(gf_estimator* h, const gf_reject_f_cfg* c);
int gf_estimator_set_state(gf_estimator* h, int frame_count, int solver_flag, const double* Ps, const double* Rs, const double* Vs,
                           const double* Bas, const double* Bgs);
int gf_estimator_get_features(gf_estimator* h, int cap, int* id, int* start_frame, int* n_obs, double* estimated_depth, int* estimate_flag,
                              int* solve_flag, int* n);
/* latest_time, latest_P, latest_Q, latest_V (estimator.h:354-356) and their wheel counterparts (estimator.h:239-242): the newest window state propagated
 * through every IMU / wheel sample received since (fastPredictIMU estimator.cpp:4014-4028 inside inputIMU :332, fastPredictWheel :4079-4093 inside inputWheel :363,
 * re-anchored by updateLatestStates :4141-4198 after every optimised frame) -- what pubLatestOdometry / pubWheelLatestOdometry publish at sensor rate.
 * imu / wheel: 16 doubles each = time, P[3], rotation matrix [9] (row-major), V[3]; either may be NULL.  Before the first optimised frame the reference
 * publishes uninitialised members; here they start at zero / identity. */
int gf_estimator_get_latest(gf_estimator* h, double* imu, double* wheel);
/* predictPtsInNextFrame / removeOutliers feedback of the last processImage (estimator.cpp:1132-1136) */
int gf_estimator_get_feedback(gf_estimator* h, int cap, int* predict_ids, double* predict_xyz, int* n_predict, int* remove_ids, int* n_remove);
int gf_estimator_get_prior(gf_estimator* h, int cap_n, int cap_blocks, int* n, int* nblocks, int* block_id, double* J, double* r);
/* single host-side steps by name (FeatureManager members, slideWindow, ...) for unit tests; see gf_estimator.hip */
int gf_estimator_debug(gf_estimator* h, const char* op, const double* in, int n_in, double* out, int cap_out, int* n_out);

/* ---- many sequences on one batched solver (not in the reference; the batched counterpart of gf_estimator_*) -------------------------------
 * n Estimators that keep the reference's single-sequence control flow and share one gf_ba handle of batch n: whenever the members that
 * are busy with a frame have all reached ceres::Solve or the marginalisation, their windows go to the device in one call.  Members take
 * feature frames (run one batched gf_tracker next to the group); IMU / wheel samples and state queries go through the member handles. */
typedef struct gf_estimator_group gf_estimator_group;
int gf_estimator_group_create(const gf_estimator_cfg* cfg, int n, gf_estimator_group** out);
/* The same group with a configuration per member: member i is an Estimator built from cfgs[i] (gf_estimator_group_create is this call with n copies of one
 * cfg).  Members may differ in everything the reference keeps per Estimator -- extrinsics tic / ric / tio / rio, sx / sy / sw, the noise parameters (acc_n,
 * gyr_n, acc_w, gyr_w and the wheel's), td*, estimate_*, extrinsic_type*, use_mcc, wdetect, stationary_detect, only_initial_with_wheel, depth_threshold,
 * init_depth, focal_length, min_parallax_px, g_norm, the GNSS thresholds -- and must agree in what sizes or schedules the shared solver: window_size,
 * gnss_enable, num_iterations, use_imu, use_wheel, depth (GF_ERR_INVALID with a message that names member and field, nothing created).  Every member needs
 * with_tracker == 0 and max_solver_time == 0.  The shared solver takes the largest max_features, max_visual and max_gnss_per_frame of the members.
 * What differs stays the member's own in the batched launches too: the device pre-integration carries the noise parameters per interval and the device
 * feature sweeps depth_threshold / init_depth / focal_length per window, so a member is the stand-alone Estimator of its cfg with either switched on. */
int gf_estimator_group_create_each(const gf_estimator_cfg* cfgs, int n, gf_estimator_group** out);
int gf_estimator_group_destroy(gf_estimator_group* g);
/* the IMU intervals a camera frame completes (the frame's own IntegrationBase and the window's, estimator.cpp:760-768, :866-869) are integrated
 * by one device launch per group step (gf_imu_preintegrate_batch's kernel) instead of on the members' host threads; results are bit-identical either way.
 * Off by default (environment GF_GROUP_DEVICE_PREINT=1 turns it on at creation): it pays on hosts with few cores, DESIGN.md section 8. */
int gf_estimator_group_set_device_preint(gf_estimator_group* g, int on);
/* FeatureManager::triangulateWithDepth (feature_manager.cpp:726-799) and Estimator::movingConsistencyCheckW (estimator.cpp:3955-3995) of all members
 * as one launch each per group step (the kernels of gf_triangulate_with_depth_batch / gf_moving_consistency_batch) instead of the members' host loops; depths, flags
 * and removed ids are bit-identical either way.  Off by default (environment GF_GROUP_DEVICE_SWEEPS=1 turns it on at creation): each launch is one more rendezvous
 * of the members, and the host loops cost ~20 us per window. */
int gf_estimator_group_set_device_sweeps(gf_estimator_group* g, int on);
int gf_estimator_group_member(gf_estimator_group* g, int i, gf_estimator** out);   /* owned by the group */
/* Estimator::inputFeature on each listed sequence, concurrently; obs = the frames back to back, n_obs[k] entries for seq[k] */
int gf_estimator_group_input_features(gf_estimator_group* g, int count, const int* seq, const double* t, const gf_feature_obs* obs, const int* n_obs);
/* The same step in two halves, as in the reference: Estimator::inputFeature only queues the frame (estimator.cpp:447-459) and processMeasurements works on it in
 * its own thread (estimator.cpp:470-560) while the tracker already handles the next image.  submit publishes the frames to the group's workers and returns;
 * wait blocks until every listed member has finished its frame and reports the first member's error.  stride >= 0: the observations of seq[k] start at
 * obs + k * stride (a tracker's padded output table as it lies: gf_tracker_track_batch*'s `out` with stride = its capacity); < 0: back to back.
 * obs / seq / n_obs stay the caller's until wait returns; one step in flight per group. */
int gf_estimator_group_submit_features(gf_estimator_group* g, int count, const int* seq, const double* t, const gf_feature_obs* obs, const int* n_obs, long long stride);
int gf_estimator_group_wait(gf_estimator_group* g);
int gf_estimator_group_stats(gf_estimator_group* g, long long* batches, long long* windows, long long* largest_batch);

/* ---- ROS-free I/O around the path: config files, trajectory output, raw frames ---------------------------------------- */
/* readParameters(std::string config_file), vins_estimator/src/estimator/parameters.cpp:138-558, plus the cam0_calib file it names
 * (PinholeCamera::Parameters::readFromYamlFile, camera_models/src/camera_models/PinholeCamera.cc:145-183; path relative to the config
 * file's directory, parameters.cpp:436-443).  Same key names and cv::FileNode defaults (a missing numeric key reads as 0).  Fills the
 * whole cfg including cfg->tracker and sets with_tracker = 1 (gnss_enable and its gnss_* keys are read, parameters.cpp:519-552).  `equalize`
 * (EQUALIZE, parameters.cpp:169; any non-zero value switches it on) sets cfg->tracker.equalize to 1.  Options outside the built path (use_line, use_yolo, plane, use_motion, num_of_cam 2, estimate_extrinsic 2,
 * gnss_local_online_sync) return GF_ERR_INVALID instead of being ignored. */
int gf_estimator_cfg_from_yaml(const char* config_file, gf_estimator_cfg* cfg);
/* readParameters (parameters.cpp:138-558) as above with the cam0_calib file read by gf_camera_from_yaml: PINHOLE, MEI and KANNALA_BRANDT files are accepted and
 * the model is handed back in *camera, for gf_estimator_set_camera.  For a model other than PINHOLE cfg->tracker gets the projection parameters as fx fy cx cy
 * and zero distortion, valid placeholders that nothing reads once the camera is set. */
int gf_estimator_cfg_from_yaml_camera(const char* config_file, gf_estimator_cfg* cfg, gf_camera_model* camera);
/* readIntrinsicParameter (feature_tracker.cpp:745-759) of an estimator that owns its tracker: gf_tracker_set_seq_camera on that tracker's one sequence, before
 * the first gf_estimator_input_image.  GF_ERR_INVALID without a tracker, and as that call refuses. */
int gf_estimator_set_camera(gf_estimator* h, const gf_camera_model* camera);
/* The two calls above for all five models (gf_camera_from_yaml_ex, gf_tracker_set_seq_camera_ex).  The placeholders of cfg->tracker for a PINHOLE_FULL file are
 * its fx fy cx cy; a SCARAMUZZA camera has no focal length: fx = fy = 1 and the centre of its affine parameters. */
int gf_estimator_cfg_from_yaml_camera_ex(const char* config_file, gf_estimator_cfg* cfg, gf_camera_model_ex* camera);
int gf_estimator_set_camera_ex(gf_estimator* h, const gf_camera_model_ex* camera);
/* show_track (SHOW_TRACK, parameters.cpp:202; what makes the node publish getTrackImage, feature_tracker.cpp:849-905 / :1047) of the same file with the same
 * reader; a missing key reads as 0.  gf_estimator_cfg does not carry it: a caller that wants the pictures turns them on (gf_estimator_set_show_track). */
int gf_show_track_from_yaml(const char* config_file, int* show_track);
/* the line pubOdometry appends to VINS_RESULT_PATH (utility/visualization.cpp:346-357): "t x y z qx qy qz qw", fixed, 9 decimals;
 * P = Ps[WINDOW_SIZE], R = Rs[WINDOW_SIZE] (row-major), quaternion as Eigen::Quaterniond(R) */
int gf_tum_append(const char* path, double t, const double* P, const double* R);
/* VINS_RESULT_PATH (output_path + "/vio.txt", parameters.cpp:347-352): creates the file empty; from then on every processed frame appends
 * its line as pubOdometry does (estimator.cpp:679 -> visualization.cpp:287-357: only once solver_flag == NON_LINEAR or the IMU was found
 * excited).  NULL or "" switches the output off. */
int gf_estimator_set_result_path(gf_estimator* h, const char* vio_txt);
/* binary PGM (P5) reader standing in for sensor_msgs::Image + cv_bridge (rosNodeTest.cpp:229-287): maxval <= 255 -> u8 (MONO8),
 * else u16 in host byte order (MONO16, depth in mm).  pixels == NULL only queries the header. */
int gf_pgm_read(const char* path, int* width, int* height, int* maxval, void* pixels, size_t cap_bytes);

/* ---- multi-GPU exchange without torch: one process per GPU, sequences sharded over the ranks, ONE collective -- the all-gather of the newest pose
 * of every window (7 doubles each) over RCCL / xGMI.  RCCL is resolved at run time (symbols already in the process, else librccl.so.1): the library itself
 * does not link against it.  The reference has no counterpart (one Estimator per process, rosNodeTest.cpp:713); this is north_star's partitioning. */
typedef struct gf_comm gf_comm;
/* rank 0 creates the 128-byte id (ncclGetUniqueId) and hands it to the other ranks out of band; every rank then builds its communicator on its device */
int gf_comm_unique_id(unsigned char* id128);
int gf_comm_create(const unsigned char* id128, int world, int rank, int device, gf_comm** out);
int gf_comm_destroy(gf_comm* c);
/* world, rank, device, the ncclComm_t and the communicator's own hipStream_t (any of them may be NULL) */
int gf_comm_info(gf_comm* c, int* world, int* rank, int* device, void** nccl_comm, void** stream);
/* all-gather of n doubles per rank between host buffers (staged through the device): recv_host = [world][n] */
int gf_comm_allgather_f64(gf_comm* c, const double* send_host, int n, double* recv_host);
/* The exchange step of the path: Ps / Rs[WINDOW_SIZE] (px py pz qx qy qz qw) of this rank's first `count` resident windows -> d_out = [world][count][7] on every
 * rank (device memory), ncclAllGather on `nccl_comm` (ncclComm_t of any owner: gf_comm_info, or torch's) enqueued on `stream` (hipStream_t) behind the solver's
 * stream.  Every rank passes the same count (the largest shard); rows behind a rank's own resident windows are zero.  Asynchronous: synchronise `stream`. */
int gf_pose_gather(gf_ba* h, void* nccl_comm, void* stream, int count, double* d_out);
/* NUMA placement: node of the GPU (/sys/bus/pci/devices/<bus id>/numa_node; -1 = none reported) and its cpulist; gf_pin_thread_to_device_node moves the calling
 * thread onto those cores (intersection with the process's affinity) and returns the node or -1; it acts when several ranks share the host (LOCAL_WORLD_SIZE > 1)
 * or GF_NUMA_PIN=1 says so, GF_NUMA_PIN=0 switches it off.  The tracker's bookkeeping pool
 * and the estimator group's workers pin themselves this way: 8 ranks x (pool + workers) on one host stay next to their own GPU. */
int gf_numa_node_of_device(int device, int* node, char* cpulist, int cap);
int gf_pin_thread_to_device_node(int device);

/* ---- ROS bag files (format 2.0) without ROS: `rosbag play <bag>` into the node's subscribers (README.md:146-187 is the only way the reference is run;
 * rosNodeTest.cpp:678-682 subscribes IMU_TOPIC / WHEEL_TOPIC / IMAGE0_TOPIC / IMAGE1_TOPIC).  Host code (ground-fusion_amd/host/rosbag_reader.h): bag records,
 * chunks (none / bz2 via libbz2.so / lz4 decoded here), index data or a scan of un-indexed chunks, connection records.  gnss_comm messages are not decoded. */
typedef struct gf_bag gf_bag;
int gf_bag_open(const char* path, gf_bag** out);
int gf_bag_close(gf_bag* b);
int gf_bag_connection_count(gf_bag* b);
/* topic / datatype of connection record i (0 .. count - 1) and its id; strings are truncated to the caller's capacity */
int gf_bag_connection(gf_bag* b, int i, int* conn_id, char* topic, int topic_cap, char* type, int type_cap);
/* the messages of the listed topics (n_topics == 0: all) in play order -- record time, ties in file order; returns their number in *count */
int gf_bag_select(gf_bag* b, const char* const* topics, int n_topics, long long* count);
/* message i of the selection: connection id, record time [s], serialized payload (valid until the next gf_bag_message / gf_bag_close on this handle) */
int gf_bag_message(gf_bag* b, long long i, int* conn_id, double* t_record, const unsigned char** data, size_t* len);
/* sensor_msgs/Imu as imu_callback reads it (rosNodeTest.cpp:567-585): header.stamp.toSec(), linear_acceleration, angular_velocity */
int gf_ros_decode_imu(const unsigned char* data, size_t len, double* t, double* acc, double* gyr);
/* nav_msgs/Odometry as wheel_callback reads it (rosNodeTest.cpp:81-189): header.stamp.toSec(), twist.twist.linear / angular, pose.pose.position (may be NULL) */
int gf_ros_decode_odometry(const unsigned char* data, size_t len, double* t, double* linear, double* angular, double* position);
/* sensor_msgs/Image -> what the node hands to trackImage.  depth == 0: getImageFromMsg (rosNodeTest.cpp:238-263): 8UC1 / mono8 copied, rgb8 / bgr8 / rgba8 /
 * bgra8 through cv_bridge::toCvCopy(MONO8) = OpenCV 4.2 cvtColor (R 4899 + G 9617 + B 1868 + 2^13) >> 14; one byte per pixel.  depth != 0:
 * getDepthImageFromMsg (:265-286): the payload relabelled MONO16; two bytes per pixel in host order.  pixels == NULL only queries t / width / height. */
int gf_ros_decode_image(const unsigned char* data, size_t len, int depth, double* t, int* width, int* height, void* pixels, size_t cap_bytes);

/* ---- stereo depth: the depth a stereo sequence's left-to-right match determines, in the eighth field of its LEFT observations -- where the reference's stereo
 * branch emits the left observations with a depth read out of the right image as if it were 16-bit millimetres (feature_tracker.cpp:344-368), which is not
 * reproduced.  With it a stereo sequence looks to everything behind the tracker like a depth-camera sequence (triangulateWithDepth, feature_manager.cpp:773).
 * DESIGN.md section 4, "Stereo depth", is the definition (csrc/gf_stereo_depth.hpp): both pixels lifted in double through the sequence's two cameras,
 * a = P_l / P_l.z, b = P_r / P_r.z, d = R b, the closed-form minimum of |s a - t - u d|^2, depth = rint(1000 s) millimetres behind six gates. */
typedef struct gf_stereo_depth_cfg {
    int enable;        /* 1: left observations of a frame with a right image carry the triangulated depth */
    int right_obs;     /* 1: the camera_id 1 observations follow as today; 0: they are not emitted (n_out counts the left ones only) */
    double R[9], t[3]; /* p_left = R p_right + t: inverse(body_T_cam0) * body_T_cam1 */
    double min_parallax, max_epipolar;   /* sine of the ray angle; normalised-plane distance in the right eye */
    double min_depth, max_depth;         /* metres; max_depth <= 65.535 */
} gf_stereo_depth_cfg;
/* what became of a point, in the order the gates are tested (the first that fires names the reason); every reason but GF_STEREO_DEPTH_OK yields depth 0 */
enum {
    GF_STEREO_DEPTH_NO_MATCH = 1,  /* status 0 */
    GF_STEREO_DEPTH_LIFT = 2,      /* a ray component that is not finite, P_l.z <= 0 or P_r.z <= 0 */
    GF_STEREO_DEPTH_PARALLAX = 3,  /* aa dd - ad^2 <= min_parallax^2 aa dd */
    GF_STEREO_DEPTH_BEHIND = 4,    /* s <= 0 or u <= 0 */
    GF_STEREO_DEPTH_EPIPOLAR = 5,  /* q = R^T (s a - t): q.z <= 0 or (q.x - b.x q.z)^2 + (q.y - b.y q.z)^2 > max_epipolar^2 q.z^2 */
    GF_STEREO_DEPTH_RANGE = 6,     /* rint(1000 s) outside [1000 min_depth, min(1000 max_depth, 65535)] */
    GF_STEREO_DEPTH_OK = 7
};
typedef struct gf_stereo_depth_stats {
    long long calls;       /* tracker calls that ran the stage for at least one sequence */
    long long launches;    /* launches of stereo_depth_kernel (one per such call; none with GF_STEREO_DEPTH_HOST=1) */
    long long points;      /* points the stage saw: cur_pts of every sequence and frame it ran for */
    long long with_depth;  /* of them, GF_STEREO_DEPTH_OK */
    long long no_match, lift, parallax, behind, epipolar, range;   /* the others, by reason */
} gf_stereo_depth_stats;
/* The switch, the rig and the gates of seq, before its first frame like the other per-sequence setters (c == NULL or enable == 0: off).  With the switch on, a
 * frame that comes with a right image returns its left observations with v[7] = (double)(int)depth_mm / 1000, the depth-camera expression; a frame handed a null
 * right entry carries 0 there for every feature; the right observations, where emitted (right_obs 1), keep -2.4.  With right_obs 0 an output sized for one eye
 * suffices.  The arithmetic runs in ONE launch of stereo_depth_kernel per call for all such sequences, behind the stereo kernel on the same stream; its rows come
 * up with the call's last copies, and the call gains no synchronisation and no copy of its own.  GF_STEREO_DEPTH_HOST=1 (read at gf_tracker_create) runs the same
 * function on the host instead, no launch; the results are the same bit for bit except through a KANNALA_BRANDT camera.  Refused by name (GF_ERR_INVALID),
 * nothing changed: a sequence without gf_tracker_set_seq_stereo, a sequence that has taken a frame or is listed by a staged one, a field that is not finite, R
 * further than 1e-9 from orthonormal with determinant +1, t == 0, a gate that is not positive, min_depth >= max_depth, max_depth > 65.535, enable or right_obs
 * outside {0, 1}.  Turning stereo off on the sequence (gf_tracker_set_seq_stereo) turns this off.  A handle on which it is never called allocates, copies and
 * launches exactly what it did without it. */
int gf_tracker_set_seq_stereo_depth(gf_tracker* h, int seq, const gf_stereo_depth_cfg* c);
/* the configuration of seq as it was set; enable == 0 and zeros if it is off */
int gf_tracker_get_seq_stereo_depth(gf_tracker* h, int seq, gf_stereo_depth_cfg* out);
/* the stage's own counters; gf_tracker_reset_stats zeroes them */
int gf_tracker_get_stereo_depth_stats(gf_tracker* h, gf_stereo_depth_stats* out);
/* The definition as a building block, through the tracker's kernel: set b of n has the cameras left[b] and right[b], the rig and gates of cfg[b] (enable and
 * right_obs are checked and otherwise not read), and the points [first[b] .. first[b + 1]): left_uv / right_uv two floats each, status a byte each.  depth_mm
 * (millimetres, 0 without a depth) and why (GF_STEREO_DEPTH_*) ARE WRITTEN, one per point.  n, first, left, right and cfg are host tables.  _device: the point
 * tables are device memory; one launch on `stream` (a hipStream_t, NULL = the null stream) whatever n, returns when it has run.  Without suffix: host tables,
 * copy in, the launch, copy out.  _host: the same function on the CPU, no device needed.  Refused (GF_ERR_INVALID, naming the set and the field): what the
 * setter refuses in a cfg, a camera gf_camera_model_ex's rules refuse, first[] not ascending from 0. */
int gf_stereo_depth_batch_device(int n, const int* first, const gf_camera_model_ex* left, const gf_camera_model_ex* right, const gf_stereo_depth_cfg* cfg,
                                 const float* d_left_uv, const float* d_right_uv, const uint8_t* d_status, uint16_t* d_depth_mm, uint8_t* d_why, void* stream);
int gf_stereo_depth_batch(int n, const int* first, const gf_camera_model_ex* left, const gf_camera_model_ex* right, const gf_stereo_depth_cfg* cfg,
                          const float* left_uv, const float* right_uv, const uint8_t* status, uint16_t* depth_mm, uint8_t* why);
int gf_stereo_depth_batch_host(int n, const int* first, const gf_camera_model_ex* left, const gf_camera_model_ex* right, const gf_stereo_depth_cfg* cfg,
                               const float* left_uv, const float* right_uv, const uint8_t* status, uint16_t* depth_mm, uint8_t* why);
/* The rig and the gates from a config file: for `num_of_cam: 2`, R and t are inverse(body_T_cam0) * body_T_cam1 (parameters.cpp:445-463, read as the estimator's
 * extrinsics are), max_depth is the file's depth_threshold, right_obs is 1, and the gates the reference has no key for get this repository's defaults:
 * min_parallax 1e-3 (about half a pixel of disparity at FOCAL_LENGTH 460), max_epipolar 10 / 460 (triangulateWithDepth's residual bound), min_depth 0.1 (below
 * it the estimator skips a depth).  Any other num_of_cam: enable == 0 and zeros.  GF_ERR_INVALID, naming the key or the field: a missing transform, and what the
 * setter refuses (a depth_threshold of 0 or beyond 65). */
int gf_stereo_depth_from_yaml(const char* config_file, gf_stereo_depth_cfg* out);
/* A stereo rig on an estimator that owns its tracker (cfg.with_tracker): gf_tracker_set_seq_stereo and gf_tracker_set_seq_stereo_depth on that tracker's one
 * sequence, before the first frame, with right_obs forced to 0 so that the back end sees one observation per feature.  From then on the estimator behaves as an
 * RGB-D one whose depths come from the matches (triangulateWithDepth, the SfM initialisation with depth, movingConsistencyCheckW); stereo reprojection factors are
 * not built.  Refused by name (GF_ERR_INVALID), nothing changed: no tracker, cfg.depth != 1 (the observations carry a depth), cfg.tracker.depth_cam != 0 (the
 * second image is a right frame), and what the two setters refuse. */
int gf_estimator_set_stereo_depth(gf_estimator* h, const gf_stereo_cfg* stereo, const gf_stereo_depth_cfg* depth);
/* Estimator::inputImage (estimator.cpp:213-242) on device frames by reference (gf_tracker_track_some_device_refs on the estimator's own tracker): img1 is the
 * depth frame of an RGB-D estimator or the right frame of a stereo one; NULL or data == NULL: none.  out / cap / n_out and the every-second-frame rule under
 * multiple_thread as gf_estimator_input_image. */
int gf_estimator_input_image_refs(gf_estimator* h, double t, const gf_frame_ref* img0, const gf_frame_ref* img1, gf_feature_obs* out, int cap, int* n_out);
/* readParameters for a stereo rig: gf_estimator_cfg_from_yaml_camera_ex that ACCEPTS `num_of_cam: 2` (cfg->tracker.depth_cam is then 0 whatever `depth` says),
 * with the right camera as gf_stereo_from_yaml and the rig as gf_stereo_depth_from_yaml read them.  With num_of_cam 1 both come back switched off.  The other
 * gf_estimator_cfg_from_yaml* entry points keep refusing num_of_cam 2. */
int gf_estimator_cfg_from_yaml_stereo(const char* config_file, gf_estimator_cfg* cfg, gf_camera_model_ex* left_camera, gf_stereo_cfg* stereo, gf_stereo_depth_cfg* stereo_depth);

#ifdef __cplusplus
}
#endif
#endif
