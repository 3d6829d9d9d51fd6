/*
 * rebvio_hip.h — C-ABI of the MI355X (gfx950) backend for rebvio's per-frame edge-detection +
 * edge-tracking hot path. Plain C types, caller-allocated outputs, int status (0 = ok, <0 = error,
 * see rebvio_hip_last_error; the codes are listed in INTEGRATION.md "Status codes"). No exceptions cross this boundary. One context per camera stream and
 * GPU; a context is not thread-safe, but its detect-side entries (detect*) and track-side entries
 * run on two private HIP streams and overlap on the device, mirroring the reference's two workers
 * (rebvio/src/rebvio.cpp:28-29).
 *
 * Each entry names the reference interface it replaces (paths relative to the reference repo).
 * The C++ classes in include/rebvio/ (EdgeDetector, EdgeMap, Core, Rebvio) are thin hosts over this
 * ABI; INTEGRATION.md shows the binding.
 */
#ifndef REBVIO_HIP_H_
#define REBVIO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: status -12 (a pair's record read before the device wrote it: sequence stamps), rebvio_hip_test_forge_record_stamp,
 *    REBVIO_HIP_DM_HEAD values compact8 / compact4 / compact1 (2: map handles outlive their context, -10)
 *    Added since, without a new version (additions only): the point-cloud entries rebvio_hip_default_cloud_filter,
 *    rebvio_hip_map_point_cloud(_async), rebvio_hip_cloud_wait / _release and their three structs; the test hook
 *    rebvio_hip_test_live_resources; the gyro-rotation entries of the streaming and batch drivers rebvio_hip_push_frame_px_gyro(_device),
 *    rebvio_hip_batch_push_px_gyro_device, the host helper rebvio_hip_gyro_integrate and the test hook rebvio_hip_test_glue_set_next;
 *    the keyframe entries rebvio_hip_map_mark_keyframe, rebvio_hip_keyframe_next, rebvio_hip_map_keyframe_matches and their struct
 *    rebvio_hip_kf_match; the keyframe snapshot and pose entries rebvio_hip_map_keyframe_snapshot, rebvio_hip_kf_snapshot_release,
 *    rebvio_hip_kf_snapshot_download, rebvio_hip_default_kf_pose_opts, rebvio_hip_map_keyframe_pose, their structs
 *    rebvio_hip_kf_pose_opts / rebvio_hip_kf_pose and the test hook rebvio_hip_test_kf_pose_host; the snapshot normals
 *    rebvio_hip_kf_snapshot_add_normals / _download_normals and the alignment entries rebvio_hip_default_kf_align_opts,
 *    rebvio_hip_map_keyframe_align, their struct rebvio_hip_kf_align_opts and the test hook rebvio_hip_test_kf_align_host; the
 *    depth fusion rebvio_hip_default_kf_fuse_opts, rebvio_hip_kf_snapshot_fuse_depth, their structs rebvio_hip_kf_fuse_opts /
 *    rebvio_hip_kf_fuse and the test hook rebvio_hip_test_kf_fuse_host; the test hook rebvio_hip_test_handover_counters;
 *    the snapshot point cloud rebvio_hip_kf_snapshot_point_cloud(_async) and the test hook rebvio_hip_test_kf_cloud_host; the
 *    batched alignment rebvio_hip_map_keyframe_align_many, its structs rebvio_hip_kf_hypothesis / rebvio_hip_kf_hyp_result, the host
 *    helpers rebvio_hip_kf_align_best / rebvio_hip_kf_hypotheses_around and the test hook rebvio_hip_test_kf_align_many_host; the depth
 *    hand-over rebvio_hip_default_kf_handover_opts, rebvio_hip_kf_snapshot_handover_depth, their structs rebvio_hip_kf_handover_opts /
 *    rebvio_hip_kf_handover and the test hook rebvio_hip_test_kf_handover_host; the edge chains and polylines
 *    rebvio_hip_map_edge_chains, rebvio_hip_default_polyline_opts, rebvio_hip_map_edge_polylines, their structs rebvio_hip_chain_ref /
 *    rebvio_hip_polyline_opts / rebvio_hip_polyline and the test hooks rebvio_hip_test_edge_chains_host /
 *    rebvio_hip_test_edge_polylines_host; the depth prior rebvio_hip_default_depth_prior_opts, rebvio_hip_map_fuse_depth_image(_device,
 *    _async), rebvio_hip_depth_prior_last_counts, their structs rebvio_hip_depth_prior_opts / rebvio_hip_depth_prior_counts and the
 *    test hook rebvio_hip_test_depth_prior_host; the stereo prior rebvio_hip_default_stereo_prior_opts, rebvio_hip_map_fuse_stereo(_async),
 *    rebvio_hip_stereo_prior_last_counts, their structs rebvio_hip_stereo_prior_opts / rebvio_hip_stereo_prior_counts and the test
 *    hooks rebvio_hip_test_stereo_prior_host / rebvio_hip_test_map_set_mask; place recognition rebvio_hip_map_place_signature,
 *    rebvio_hip_place_db_create / _release / _clear / _size / _add / _add_signature / _entry / _query / _query_signature, their
 *    struct rebvio_hip_place_match and the test hooks rebvio_hip_test_place_signature_host / rebvio_hip_test_place_query_host; the
 *    straight segments rebvio_hip_default_segment_opts, rebvio_hip_map_edge_segments, their structs rebvio_hip_segment_opts /
 *    rebvio_hip_line_segment / rebvio_hip_segment_counts and the test hook rebvio_hip_test_edge_segments_host. */
#define REBVIO_HIP_ABI_VERSION 3

/* Host mirror of one keyline: field-for-field rebvio::types::KeyLine
 * (rebvio/include/rebvio/types/keyline.hpp:24-40), 84 bytes. Device storage is SoA. */
typedef struct rebvio_hip_keyline {
  float pos[2];
  float pos_img[2];
  float match_pos_img[2];
  float gradient[2];
  float match_gradient[2];
  float gradient_norm;
  float match_gradient_norm;
  float rho;
  float sigma_rho;
  int id;
  int id_prev;
  int id_next;
  int match_id;
  int match_id_forward;
  int match_id_keyframe;
  unsigned int matches;
} rebvio_hip_keyline;

/* Camera constants (camera.hpp:61-72), EdgeDetectorConfig (edge_detector.hpp:19-32), CoreConfig
 * (core.hpp:82-95), EdgeMapConfig (edge_map.hpp:19-26), gyro noise of ImuStateConfig
 * (types/imu.hpp:158-159). */
typedef struct rebvio_hip_params {
  int rows, cols;
  float fm, cx, cy;
  int keylines_ref, keylines_max;
  float pos_neg_threshold, dog_threshold, threshold, gain, max_threshold, min_threshold;
  float search_range, reweight_distance, match_treshold;
  unsigned int min_match_threshold, iterations, global_min_matches_threshold;
  float pixel_uncertainty, quantile_cutoff;
  int quantile_num_bins;
  float reshape_q_abs;
  float pixel_uncertainty_match, match_threshold_norm, match_threshold_angle, regularization_threshold;
  float gyro_std_dev, gyro_bias_std_dev;
  int device_id;  /* HIP device ordinal for this camera stream */
  int map_pool;   /* edge maps kept alive at once (>= 3: old, new, in-flight detect); 0 = default */
} rebvio_hip_params;

typedef struct rebvio_hip_ctx rebvio_hip_ctx;
typedef struct rebvio_hip_map rebvio_hip_map;

/* Result of one frame-pair step (rebvio.cpp:142-259 without accelerometer/SAB fusion). */
typedef struct rebvio_hip_pair_out {
  float Vg[3];
  float P_Vg[9];
  float F;
  float Xv[6];
  float W_Xv[36];
  float Xgv[6];
  float V[3];
  float R[9];
  float P_V[9];
  float sigma_rho_min;
  int ext_ok;
  int klm_num;
  int kf_matches;
  int reg_num;
  int lm_accept_mask;
  int status; /* 0 ok, 1 minimization NaN, 2 insufficient matches */
} rebvio_hip_pair_out;

int rebvio_hip_abi_version(void);
const char* rebvio_hip_last_error(void);

/* Defaults of the reference's config structs and Camera() for a rows x cols sensor. */
void rebvio_hip_default_params(rebvio_hip_params* p, int rows, int cols);

/* Replaces the constructors EdgeDetector(camera, config) (edge_detector.cpp:17-26), ScaleSpace /
 * FastGaussian (scale_space.cpp:14-41,184-190), Core(camera, config) + DistanceField (core.cpp:17-24,
 * core.hpp:22-28): allocates every device buffer once.
 * Sensor sizes: rows, cols >= 32, any width (the integral images get a row pitch of cols rounded up to 4 internally),
 * cols <= 4096, rows <= 2548 (LDS-staged scan strips); -3 otherwise.
 * Also -3: search_range > 255 or search_range + 2 * pixel_uncertainty_match >= 258 (per-wave probe sequence buffer),
 * quantile_num_bins outside 1..128, keylines_max * 2 * search_range >= 2^23 (distance-field key encoding),
 * keylines_max outside 1..65536 (the LM reduction stages at most 256 record groups of 256 keylines in LDS).
 * Also -3, here and in rebvio_hip_batch_create, before a device is queried: a search_range that is not a whole number of pixels.
 * The field kernels walk r over [-(int)search_range, (int)search_range); the reference's loop runs up to the float itself
 * (core.hpp:49) and takes one step more for a fractional range, so only whole numbers give the reference's field.
 * Also -3 (rebvio_hip_last_error names the fields), checked with the rest before a device is queried, here and in
 * rebvio_hip_batch_create: detection parameters whose gradient gate cannot reject a zero gradient. The gate keeps a candidate
 * unless g2 < (thr * 765 * dog_threshold)^2 (edge_detector.cpp:70,107), and the lowest thr the servo hands it is
 *   lo = min(min_threshold, max_threshold) with gain > 0 (both clamps apply on every frame),  lo = threshold otherwise.
 * Required: pos_neg_threshold, dog_threshold, threshold, gain, min_threshold and max_threshold finite; pos_neg_threshold >= 0;
 * (lo * 765 * dog_threshold)^2 > 0, evaluated in fp32 as the kernels spell it. Why: with a bound of zero a pixel of a flat region
 * passes every gate with a zero gradient (theta2 / 0 is NaN and fabs(NaN) > 0.5 is false), its keyline gets a NaN position, and
 * the reference's joinEdges indexes its mask with that position (edge_detector.cpp:125-165: it writes outside the mask; the
 * same parameters crash the CPU oracle of the tests). min_threshold > max_threshold is legal: the servo's threshold then takes
 * only these two values (max_threshold whenever it is above it, min_threshold otherwise). */
int rebvio_hip_create(const rebvio_hip_params* p, rebvio_hip_ctx** out);
void rebvio_hip_destroy(rebvio_hip_ctx* ctx);

/* ScaleSpace::build (scale_space.cpp:203-208) on a host fp32 image (0..765); any output may be NULL.
 * Test/diagnostic entry: detect() runs the same kernels without the downloads. */
int rebvio_hip_scale_space(rebvio_hip_ctx* ctx, const float* img_host, float* scale0, float* scale1, float* dog,
                           float* mag);

/* EdgeDetector::detect (edge_detector.cpp:30-43): threshold servo, buildEdgeMap, joinEdges,
 * tuneThreshold. The image is the undistorted fp32 frame the reference passes in types::Image
 * (rebvio.cpp:43-47). Returns a pooled map (release with rebvio_hip_map_release). Asynchronous: the
 * keyline count is fetched by rebvio_hip_map_size. */
int rebvio_hip_detect(rebvio_hip_ctx* ctx, const float* img_host, size_t pitch_bytes, uint64_t ts_us,
                      rebvio_hip_map** out);
/* Same, for a u8 frame already resident in device memory: fuses convertTo(CV_32F, 3.0) (rebvio.cpp:43)
 * into the first scan kernel. `frame_dev` is a device pointer to rows*cols bytes, dense. */
int rebvio_hip_detect_u8_device(rebvio_hip_ctx* ctx, const uint8_t* frame_dev, uint64_t ts_us, rebvio_hip_map** out);
/* Same, for a u8 frame in host memory (the MONO8 image ros_rebvio hands to imageCallback, ros_rebvio.cpp:96-104):
 * uploads 1 byte/pixel instead of the fp32 frame. */
int rebvio_hip_detect_u8(rebvio_hip_ctx* ctx, const uint8_t* img_host, size_t pitch_bytes, uint64_t ts_us,
                         rebvio_hip_map** out);
/* Lens model of the front end (camera.hpp:39-40,54-58: cv::undistort(in, out, K(fm,0,cx;0,fm,cy), D(k1,k2,p1,p2,k3))).
 * K4 = fx, fy, cx, cy; D5 = k1, k2, p1, p2, k3. Once set, every *_u8 detect entry runs convertTo(CV_32F,3.0) +
 * undistort on the device before the scale space (rebvio.cpp:43-47); all-zero D5 switches it off. Synchronises.
 * A K4 or D5 word that is not finite, or a focal length that is not positive, is refused with -3 before the context is
 * touched, an all-zero D5 included: the model in force stays. Source coordinates saturate as OpenCV's maps do (a pixel whose
 * source lies beyond +-2^31 / 32 px, or is a NaN, reads the constant border 0). */
int rebvio_hip_set_undistort(rebvio_hip_ctx* ctx, const float K4[4], const float D5[5]);
/* The front end alone: u8 host frame -> undistorted fp32 host frame (rows*cols floats). Needs a lens model. */
int rebvio_hip_front_end_u8(rebvio_hip_ctx* ctx, const uint8_t* img_host, float* out_host);
/* Pixel formats of the *_px entries: the frame's grey byte is formed on the device, fused into the first scan pass (or into
 * the lens front end), then x3 as for a MONO8 frame, so everything downstream sees the values of the grey frame.
 *   GRAY8          1 byte/px   the byte (the *_u8 entries)
 *   RGB8 / BGR8    3 bytes/px  (R*4899 + G*9617 + B*1868 + 8192) >> 14 (cv::cvtColor RGB2GRAY / BGR2GRAY, what cv_bridge's
 *                              MONO8 conversion computes)
 *   RGBA8 / BGRA8  4 bytes/px  the same, alpha ignored
 *   YUYV           2 bytes/px  Y; bytes Y0 U Y1 V (cv::COLOR_YUV2GRAY_YUY2, UVC webcams)
 *   UYVY           2 bytes/px  Y; bytes U Y0 V Y1 (ROS "yuv422", cv::COLOR_YUV2GRAY_UYVY)
 * YUYV / UYVY frames need an even width. Device frames are dense (rows of cols * bytes/px); host frames take pitch_bytes >=
 * cols * bytes/px (0 = dense). With cols a multiple of 4 the first pass reads a lane's four pixels as one 8-, 12- or 16-byte
 * load: a device frame should start 16-byte aligned (as hipMalloc'd memory does). The format is an argument
 * of each call: one stream may change it from frame to frame. Every
 * _px entry checks its arguments before it touches the device and refuses (-3, rebvio_hip_last_error says why) an unknown
 * format, an odd width for YUYV / UYVY, a pitch below a row's bytes and a null frame. GRAY8 through a _px entry is the
 * matching _u8 entry. */
#define REBVIO_HIP_PX_GRAY8 0
#define REBVIO_HIP_PX_RGB8 1
#define REBVIO_HIP_PX_BGR8 2
#define REBVIO_HIP_PX_RGBA8 3
#define REBVIO_HIP_PX_BGRA8 4
#define REBVIO_HIP_PX_YUYV 5
#define REBVIO_HIP_PX_UYVY 6
int rebvio_hip_detect_px(rebvio_hip_ctx* ctx, const void* img_host, size_t pitch_bytes, int fmt, uint64_t ts_us, rebvio_hip_map** out);
int rebvio_hip_detect_px_device(rebvio_hip_ctx* ctx, const void* frame_dev, int fmt, uint64_t ts_us, rebvio_hip_map** out);
/* rebvio_hip_front_end_u8 for a frame of any format (host memory, pitch_bytes 0 = dense). Needs a lens model. */
int rebvio_hip_front_end_px(rebvio_hip_ctx* ctx, const void* img_host, size_t pitch_bytes, int fmt, float* out_host);
/* Detection masks: where keylines may come from. One byte per pixel in the coordinates of the image the scale space sees (with a
 * lens model: UNDISTORTED coordinates); non-zero = "keylines may come from here", as OpenCV's mask arguments (a torch bool or
 * uint8 tensor has this layout). A masked pixel is skipped in buildEdgeMap (edge_detector.cpp:73-121) exactly like one that
 * fails the magnitude test; nothing else changes: the scale space, DoG and gradient cover the whole frame, keylines_max counts
 * the surviving candidates in raster order, joinEdges links surviving keylines only, tuneThreshold and the threshold servo see
 * the masked keyline count, tracking is untouched. Two kinds, which may be combined (a pixel must then pass both):
 *  - the static mask of a context, rebvio_hip_set_detection_mask: copied to the device (the caller's buffer is free when the call
 *    returns; pitch_bytes >= cols, 0 = dense; NULL clears it). It applies to every detect and push entry of the context from the
 *    next frame on; frames already queued keep the mask they were queued with (the call waits until their candidate kernels
 *    have run before it rewrites the device copy). A batch lane's static mask is set on rebvio_hip_batch_lane(b, l) and is
 *    picked up by the batch's next push.
 *  - a per-frame mask in device memory (dense, rows*cols bytes), with device-resident frames only: the *_masked_device entries.
 *    The device reads it (and the frame) on the library's streams after the call returns: keep both unchanged until the frame's
 *    detection has finished. A point the caller can rely on: once rebvio_hip_map_size (or any other call that waits for the map)
 *    has returned for a detect entry's map; for a push entry, once the record of the pair that ends at this frame has been
 *    handed out (push, next_record or flush).
 * The masked entries refuse (-3, rebvio_hip_last_error says why) before anything is queued: a null frame or mask, an unknown
 * pixel format, a host pitch below cols; a bad frame as their unmasked *_px_device twins do. */
int rebvio_hip_set_detection_mask(rebvio_hip_ctx* ctx, const uint8_t* mask_host, size_t pitch_bytes);
int rebvio_hip_detect_px_masked_device(rebvio_hip_ctx* ctx, const void* frame_dev, int fmt, const uint8_t* mask_dev, uint64_t ts_us,
                                       rebvio_hip_map** out);
/* config_->threshold after the servo and auto_threshold_ (edge_detector.hpp:84,91). Synchronises. */
int rebvio_hip_detector_state(rebvio_hip_ctx* ctx, float* threshold, float* auto_threshold, int* keylines_count);

/* EdgeMap accessors (edge_map.hpp:40-75). size/threshold synchronise with the detect stream. */
int rebvio_hip_map_size(rebvio_hip_map* m);
float rebvio_hip_map_threshold(rebvio_hip_map* m);
uint64_t rebvio_hip_map_ts(rebvio_hip_map* m);
/* Lazy host mirror of keylines() / mask() (edge_map.hpp:50,75): AoS keylines (may be NULL) and the
 * dense image-index -> keyline-index table (may be NULL; -1 = none). A map fresh from detect() only waits for its own detection;
 * once a tracking call has been given the map the download waits for the track stream as well. Downloading a map from one
 * thread WHILE another thread's tracking call works on it mirrors some state in between (as reading a reference EdgeMap
 * during its tracking step would). */
int rebvio_hip_map_download(rebvio_hip_map* m, rebvio_hip_keyline* keylines, int* mask);
/* Edge image for registerEdgeImageCallback consumers, rendered on the device the way ros_rebvio.cpp:32-50 draws it on
 * the host: the grey frame (rows*cols bytes, NULL = black) replicated to RGB, each keyline's pixel
 * (round(pos[1]), round(pos[0])) set to (255,0,0). rgb_out = rows*cols*3 bytes. Synchronises. */
int rebvio_hip_render_edge_image(rebvio_hip_map* map, const uint8_t* gray_host, uint8_t* rgb_out_host);

/* The depth-bearing keylines of a map as a packed point cloud, extracted on the device by kernels of their own (an
 * order-preserving compaction over the map's keyline arrays; nothing of the tracking kernels changes). No reference counterpart:
 * it is what regularize1Iter / updateInverseDepth (edge_map.cpp:220-259, core.cpp:417-456) are run for.
 * A keyline passes the filter when ALL of
 *   matches >= min_matches,  rho >= rho_min,  rho <= rho_max,  sigma_rho <= max_rel_sigma * rho   (one rounded fp32 multiply)
 * hold (a NaN in rho or sigma_rho fails them). A filter with rho_min <= 0, rho_min > rho_max, max_rel_sigma < 0 or a NaN field is
 * refused (-3), so rho > 0 for every point. With fm of the context's parameters and pos_img the principal-point coordinates
 * rotateKeylines works on (edge_map.cpp:60), every operation one IEEE fp32 operation in this order, no contraction:
 *   u = pos_img[0] / fm;  v = pos_img[1] / fm;  z = scale / rho;  xc = u * z;  yc = v * z;  zc = z;
 *   xyz[i] = ((R[3i] * xc + R[3i+1] * yc) + R[3i+2] * zc) + t[i]
 * pose NULL = identity, zero, 1. Points come in ascending keyline index; `keyline` is strictly increasing and the cloud is
 * reproducible bit for bit. *count = keylines that pass; min(count, cap) records are written (a cap below count is no error).
 * State: the cloud shows the map's keylines as they are when the extraction runs in stream order (the rule of
 * rebvio_hip_map_download). So a map that has since served as a pair's OLD map has been rotated into the newer frame by that pair;
 * and a map handed to rebvio_hip_track_pair_finish_async with R_prior_next is already rotated for the next pair when its second
 * half ends: until the next _begin has consumed that promise both entries refuse it (-7) rather than return a cloud in a frame the
 * caller did not ask for. */
typedef struct rebvio_hip_cloud_point {
  float xyz[3];        /* position, see above */
  float rho;           /* KeyLine::rho as stored */
  float sigma_rho;     /* KeyLine::sigma_rho as stored */
  float gradient_norm; /* KeyLine::gradient_norm ("intensity" for PointCloud2 consumers) */
  int keyline;         /* index of the source keyline in its map */
  unsigned int matches; /* KeyLine::matches */
} rebvio_hip_cloud_point;
typedef struct rebvio_hip_cloud_filter {
  unsigned int min_matches;
  float max_rel_sigma, rho_min, rho_max;
} rebvio_hip_cloud_filter;
typedef struct rebvio_hip_cloud_pose {
  float R[9]; /* row-major */
  float t[3];
  float scale;
} rebvio_hip_cloud_pose;
typedef struct rebvio_hip_cloud rebvio_hip_cloud;
/* min_matches 2, max_rel_sigma 0.5, rho in [1e-3, 20] (the bounds KeyLine::rho is clamped to; DESIGN.md 5e says why). */
void rebvio_hip_default_cloud_filter(rebvio_hip_cloud_filter* f);
/* Synchronous: waits for everything queued that concerns the map (like rebvio_hip_render_edge_image), extracts, and returns the
 * cloud in caller memory (points_host: cap records; may be NULL with cap 0: only the count). filter NULL = the default filter.
 * -3: null map / count, negative cap, null points with cap > 0, invalid filter, NaN in the pose - all checked before the device
 * is touched; -10: the map's context has been destroyed; -7: see "State" above.
 * Although it takes a map alone, this entry is a TRACK-side entry like the queued one below: the extraction runs on the track
 * stream, so it is called from the context's tracking thread (not concurrently with a tracking call), unlike
 * rebvio_hip_map_download / _render_edge_image. Once a cloud of a map has been extracted the map counts as used by the tracker:
 * later rebvio_hip_map_download calls on it wait for the track stream as well. */
int rebvio_hip_map_point_cloud(rebvio_hip_map* map, const rebvio_hip_cloud_filter* filter, const rebvio_hip_cloud_pose* pose,
                               rebvio_hip_cloud_point* points_host, int cap, int* count);
/* Queued: the extraction goes on the TRACK stream in call order and the call returns at once. Called between _finish_async(k) and
 * _begin(k+1) it sees map k exactly as pair k left it, without the host waiting for anything. The records are extracted into device
 * memory (capacity keylines_max); a kernel on a stream of its own then writes exactly those that exist into host-visible memory,
 * the count and a sequence stamp behind them - no copy of `capacity` records for a count the host does not have yet.
 * rebvio_hip_cloud_wait blocks until that extraction has run: *points = host-readable records, valid until the release;
 * *device_points = the records in device memory, for consumers that stay on the GPU (either may be NULL). A cloud
 * whose stamp is not the extraction's own - read before it was written - is -12, never stale points. -10 after
 * rebvio_hip_destroy. rebvio_hip_cloud_release returns the buffer to a small pool of the context (exactly once per handle; safe
 * after rebvio_hip_destroy). */
int rebvio_hip_map_point_cloud_async(rebvio_hip_ctx* ctx, rebvio_hip_map* map, const rebvio_hip_cloud_filter* filter,
                                     const rebvio_hip_cloud_pose* pose, rebvio_hip_cloud** out);
int rebvio_hip_cloud_wait(rebvio_hip_cloud* cloud, const rebvio_hip_cloud_point** points, int* count, const void** device_points);
void rebvio_hip_cloud_release(rebvio_hip_cloud* cloud);

/* Edge chains. joinEdges links every keyline to its neighbours along the edge (id_prev / id_next, edge_detector.cpp:125-165), but the
 * links are not a clean list: id_next is many-to-one, id_prev keeps one claimant, closed contours exist, and an uploaded map
 * (rebvio_hip_map_upload) may hold any integers in the two fields. With n the map's size:
 *   succ(i) = id_next[i] when 0 <= id_next[i] < n, id_next[i] != i and id_prev[id_next[i]] == i; otherwise succ(i) = -1.
 *   pred(j) = the unique i with succ(i) == j, otherwise -1.
 * The components of succ are simple paths and simple cycles; no out-of-range value is ever used as an index. One record per keyline:
 *   head    for a path the member with pred == -1; for a cycle the smallest member index
 *   rank    the number of succ steps from head
 *   length  the number of members
 *   flags   bit 0: the chain is cyclic
 * Chain table: chains are numbered c = 0..C-1 by ascending head; starts[c] = the sum of the lengths in front of chain c,
 * starts[C] = n; order[starts[c] + rank] = keyline; order is a permutation of 0..n-1.
 * rebvio_hip_map_edge_chains: *n_keylines = n, *n_chains = C (either may be NULL); min(n, cap_keylines) records of refs_host and of
 * order_host and min(C + 1, cap_chains) entries of starts_host are written (cap_chains counts the ints of starts_host; any output
 * pointer may be NULL, a cap below the count is no error). -3: null map, a negative cap.
 * Synchronous and track-side, exactly as rebvio_hip_map_point_cloud: the track stream, its state rule, -7 for a map promised to
 * R_prior_next, -10 after rebvio_hip_destroy (the chains read only the two link fields, which tracking never writes; the rules are
 * kept the same for simplicity). Everything is integer work and reproducible bit for bit.
 * Launches, fixed per context whatever n and the links are (an empty map launches the same): with R = ceil(log2(keylines_max))
 *   rebvio_hip_map_edge_chains     1 k_chain_link + R k_chain_round + k_chain_rank + k_chain_count + k_chain_emit + k_chain_order = R + 5
 *   rebvio_hip_map_edge_polylines  the same R + 5, then k_poly_count + k_poly_emit + k_poly_lines                                 = R + 8
 * No workgroup waits for another inside a kernel; every dependency is a kernel boundary; sizes are read on the device. Scratch is one
 * allocation per context, made at the first call of either entry that reaches the device (about 124 bytes per keylines_max). */
typedef struct rebvio_hip_chain_ref { /* 16 bytes */
  int head, rank, length, flags;
} rebvio_hip_chain_ref;
int rebvio_hip_map_edge_chains(rebvio_hip_map* map, rebvio_hip_chain_ref* refs_host, int cap_keylines, int* order_host, int* starts_host,
                               int cap_chains, int* n_keylines, int* n_chains);
/* Polylines: the chains as ordered 3D curves. Slot s = starts[c] + rank is kept when its keyline passes the cloud filter (the test of
 * rebvio_hip_map_point_cloud, bit for bit) and its chain's length >= min_chain_length. A line is a maximal run of kept, consecutive
 * slots of one chain; a run never wraps from a cyclic chain's last rank to rank 0. Points come out in slot order as
 * rebvio_hip_cloud_point, with the formula, operation order and `keyline` field of a map's cloud: a point is byte-identical to that
 * keyline's record from rebvio_hip_map_point_cloud under the same filter and pose. refs2_host (may be NULL) takes {head, rank} per
 * point, two ints each. One record per line; first_point indexes the full sequence of points (cap_points does not shift it); bit 0 of
 * flags is "closed": the chain is cyclic and the line is all of it.
 * *n_points / *n_lines = all of them; min(n_points, cap_points) points and min(n_lines, cap_lines) lines are written. opts NULL = the
 * defaults (the default cloud filter, min_chain_length 8); pose NULL = identity. -3, before the device is touched: null map, n_points
 * or n_lines, min_chain_length < 1, an invalid filter, a NaN in the pose, a negative cap, null points_host with cap_points > 0, null
 * lines_host with cap_lines > 0. Otherwise the rules of rebvio_hip_map_edge_chains (and the "State" rule of the cloud: -7). */
typedef struct rebvio_hip_polyline_opts {
  rebvio_hip_cloud_filter filter;
  int min_chain_length;
  int reserved;
} rebvio_hip_polyline_opts;
typedef struct rebvio_hip_polyline { /* 16 bytes */
  int first_point; /* index of the line's first point */
  int points;      /* its number of points */
  int head;        /* head of its chain */
  int flags;       /* bit 0: closed */
} rebvio_hip_polyline;
void rebvio_hip_default_polyline_opts(rebvio_hip_polyline_opts* o);
int rebvio_hip_map_edge_polylines(rebvio_hip_map* map, const rebvio_hip_polyline_opts* opts, const rebvio_hip_cloud_pose* pose,
                                  rebvio_hip_cloud_point* points_host, int* refs2_host, int cap_points, rebvio_hip_polyline* lines_host,
                                  int cap_lines, int* n_points, int* n_lines);
/* Test hooks: the same per-step statements on the host (rebvio_amd/csrc/edge_chains.hpp), from plain arrays, no device. The
 * arguments and results of the two entries above, with id_prev / id_next (n ints each) or n keylines in place of the map, and fm in
 * place of the context's. -3 as there, and for a negative n or a null input with n > 0. */
int rebvio_hip_test_edge_chains_host(const int* id_prev, const int* id_next, int n, rebvio_hip_chain_ref* refs, int cap_keylines,
                                     int* order, int* starts, int cap_chains, int* n_keylines, int* n_chains);
int rebvio_hip_test_edge_polylines_host(float fm, const rebvio_hip_keyline* keylines, int n, const rebvio_hip_polyline_opts* opts,
                                        const rebvio_hip_cloud_pose* pose, rebvio_hip_cloud_point* points, int* refs2, int cap_points,
                                        rebvio_hip_polyline* lines, int cap_lines, int* n_points, int* n_lines);

/* Straight segments: the polylines split where they bend, each straight piece with two 3D end points whose depths come from all of
 * the piece's keylines at once (along the image of a 3D straight line inverse depth is an affine function of image position).
 * Input: the polylines of the map under opts.poly. Points are 0..np-1 in slot order, lines are the maximal runs, q[p] is the pos_img
 * of point p's keyline. A line of one point has no segment; a closed line is treated as the open run from its first to its last point.
 * State: every point is a vertex, or interior to a segment [a, b] with a < p < b. Initially a line's first and last points are vertices
 * and every other point is interior to [first, last].
 * One split round, for every interior point p - every * / + - is one fp32 operation in this order, nothing contracted:
 *   ex = q[b].x - q[a].x; ey = q[b].y - q[a].y; px = q[p].x - q[a].x; py = q[p].y - q[a].y;
 *   l2 = ex*ex + ey*ey; cr = ex*py - ey*px;
 *   d2 = (l2 == 0) ? px*px + py*py : (cr*cr) / l2; if (!(d2 >= 0)) d2 = 0;          (a NaN position never splits)
 * The segment's winner is the point with the largest d2, a tie goes to the lowest p: the 64-bit maximum of the keys
 * (bits(d2) << 32) | (0xFFFFFFFF - p), which are distinct - the result does not depend on the order the maximum is taken in. If the
 * winner's d2 > tol * tol (one fp32 multiply) the winner m becomes a vertex: points of (a, m) get b = m, points of (m, b) get a = m.
 * Rounds are level-synchronous: every segment that exists at the start of a round is tested once in it. max_rounds rounds are
 * launched; rounds_used is the number of rounds in which something split. After the last round one more measuring pass leaves every
 * segment's max_dev2 (its winner's d2, or 0 with no interior point); the segment is unresolved if max_dev2 is still > tol * tol.
 * Segments are numbered in point order: every vertex that is not its line's last point begins one; adjacent segments share their
 * vertex. A segment is kept when points = b - a + 1 >= min_points and l2 >= min_length * min_length (one fp32 multiply); only kept
 * segments are emitted, in order.
 * Depth fit of a kept segment over its members i = 0..points-1 (p = a + i, both ends included). In fp32: t = (px*ex + py*ey) / l2.
 * Then in fp64: sg = fabsf(sigma_rho); if (!(sg >= 1e-6f)) sg = 1e-6f; w = 1.0 / ((double)sg * sg); r = (double)rho;
 *   wt = w*t; wr = w*r; the six terms are w, wt, wt*t, wr, wt*r, wr*r and their sums Sw, Swt, Swtt, Swr, Swtr, Swrr.
 * Each sum is 16 partial sums: partial j adds the members i = j, j+16, ... in ascending order, starting from +0.0; the 16 partials are
 * combined as the pairwise tree ((p0+p1)+(p2+p3)) + ... - this order is part of the definition.
 *   det = Sw*Swtt - Swt*Swt; r0 = (Swtt*Swr - Swt*Swtr) / det; sl = (Sw*Swtr - Swt*Swr) / det; r1 = r0 + sl;
 *   v0 = Swtt / det; v1 = ((Swtt - 2*Swt) + Sw) / det; chi2 = Swrr - (r0*Swr + sl*Swtr); if (!(chi2 > 0)) chi2 = 0;
 * Depth valid (positive tests, a NaN fails): det > 0, v0 >= 0, v1 >= 0 and (float)r0, (float)r1 both in the filter's
 * [rho_min, rho_max]. When valid rho0 / rho1 = (float)r0 / r1, sigma_rho0 / 1 = (float)sqrt(v0 / v1) and xyz0 / xyz1 = the point of
 * a map's cloud at q[a] / q[b] with rho0 / rho1 (same formula, operation order and pose); otherwise those ten floats are 0.
 * counts: segments_all and unresolved count every segment, kept and depth_valid the kept ones (whatever cap_segments is); points and
 * lines are the polylines' counts. min(kept, cap_segments) records are written; a cap below the count is no error. opts NULL = the
 * defaults (the polyline defaults, tol 1, min_length 4, min_points 8, max_rounds 16); pose NULL = identity. -3, before the device is
 * touched: everything rebvio_hip_map_edge_polylines refuses in opts.poly and the pose, a negative or NaN tol or min_length,
 * min_points < 2, max_rounds outside 1..32, null counts, a negative cap_segments, null segs_host with cap_segments > 0. Otherwise
 * the rules of rebvio_hip_map_edge_polylines: synchronous, track-side, -7, -10.
 * Launches, fixed per context and max_rounds whatever the map holds: the polylines' R + 8, then 2 * max_rounds + 5 (k_seg_init,
 * max_rounds x (k_seg_far + k_seg_split), the measuring k_seg_far, k_seg_count, k_seg_emit, k_seg_fit). A round behind a round
 * in which nothing split returns at once. Scratch is one more allocation per context, made at this entry's first call that
 * reaches the device (about 132 bytes per keylines_max). */
typedef struct rebvio_hip_segment_opts {
  rebvio_hip_polyline_opts poly;
  float tol;        /* px: the largest deviation a segment keeps */
  float min_length; /* px: between the two end points */
  int min_points;   /* >= 2 */
  int max_rounds;   /* 1..32 */
} rebvio_hip_segment_opts;
typedef struct rebvio_hip_line_segment { /* 80 bytes */
  float xyz0[3], xyz1[3];
  float uv0[2], uv1[2]; /* q[a], q[b] */
  float rho0, rho1, sigma_rho0, sigma_rho1, max_dev2, chi2;
  int first_point; /* a: index into the polylines' points */
  int points;
  int line;
  int flags; /* bit 0: depth valid; bit 1: unresolved */
} rebvio_hip_line_segment;
typedef struct rebvio_hip_segment_counts {
  int segments_all, kept, depth_valid, unresolved, rounds_used, points, lines, reserved;
} rebvio_hip_segment_counts;
void rebvio_hip_default_segment_opts(rebvio_hip_segment_opts* o);
int rebvio_hip_map_edge_segments(rebvio_hip_map* map, const rebvio_hip_segment_opts* opts, const rebvio_hip_cloud_pose* pose,
                                 rebvio_hip_line_segment* segs_host, int cap_segments, rebvio_hip_segment_counts* counts);
/* Test hook: the same statements on the host (rebvio_amd/csrc/edge_segments.hpp) over the host polylines of n keylines. */
int rebvio_hip_test_edge_segments_host(float fm, const rebvio_hip_keyline* keylines, int n, const rebvio_hip_segment_opts* opts,
                                       const rebvio_hip_cloud_pose* pose, rebvio_hip_line_segment* segs, int cap_segments,
                                       rebvio_hip_segment_counts* counts);

/* Keyframes. Every keyline carries match_id_keyframe, "ID of the matching keyline in the last keyframe" (types/keyline.hpp:39):
 * forwardMatch and directedMatch copy it from the matched keyline of the old map (edge_map.cpp:93,210) and directedMatch counts the
 * keylines that still hold one into kf_matches (edge_map.cpp:212). Detection writes -1 and the reference never sets anything else,
 * so kf_matches is 0 until a map is MARKED: match_id_keyframe[i] = i for every keyline i of the map - the map becomes the keyframe,
 * and from then on the field tells, in every later map of the stream, which keyline of the keyframe a keyline continues, and
 * kf_matches / keylines how much of the keyframe is still alive (the usual signal for choosing the next one).
 * Mark a map AFTER it has been a pair's new map and BEFORE it serves as an old map: being tracked as a new map overwrites the ids of
 * its matched keylines with those of the previous keyframe (that is the field's meaning in the reference).
 * rebvio_hip_map_mark_keyframe queues one kernel on the TRACK stream in call order and returns at once; it waits for nothing on the
 * host. Nothing else of the map changes. A track-side entry like rebvio_hip_map_point_cloud_async: allowed between stepwise calls,
 * between rebvio_hip_track_pair calls and between _finish_async(k) and _begin(k+1). The ids do not depend on the keylines' frame, so
 * a map promised to R_prior_next is marked like any other (no -7). The map counts as used by the tracker afterwards (see
 * rebvio_hip_map_download). -3: null context or map, a map of another context; -10: the context has been destroyed - all checked
 * before the device is touched. */
int rebvio_hip_map_mark_keyframe(rebvio_hip_ctx* ctx, rebvio_hip_map* map);
/* Keyframe-to-current correspondences of a map. A keyline i of the map is a claimant of keyframe slot j when
 * 0 <= match_id_keyframe[i] == j < kf_size (ids of -1 or >= kf_size are ignored; kf_size = the keyframe map's size). Per slot with at
 * least one claimant one record, in ascending kf_keyline: the number of claimants and the winner - the claimant of smallest key
 * (sk << 32) | i with sk = the bits of sigma_rho + 0.0f when sigma_rho >= 0, 0xFFFFFFFF otherwise (NaN, negative): the smallest
 * sigma_rho wins, the smallest index among equals. *count = such slots; min(count, cap) records are written (a cap below count is no
 * error). Bit-reproducible: the only atomics are a 64-bit minimum and an integer add per slot, both independent of order.
 * Synchronous and track-side, exactly as rebvio_hip_map_point_cloud: the map's keylines as they are when the kernels run in stream
 * order, called from the tracking thread, and the map counts as used by the tracker afterwards. kf_size 0: count 0, nothing is
 * launched. -3, before the device is touched: null map or count, negative cap, null out_host with cap > 0, kf_size outside
 * 0..keylines_max; -10: the context has been destroyed; -7: the map is promised to R_prior_next (the record carries pos_img; see
 * "State" of the point-cloud entries). */
typedef struct rebvio_hip_kf_match { /* 32 bytes */
  int kf_keyline;       /* index in the keyframe map */
  int keyline;          /* index in THIS map of the winning claimant */
  int claimants;        /* keylines of this map with match_id_keyframe == kf_keyline */
  unsigned int matches; /* winner's KeyLine::matches */
  float rho, sigma_rho; /* winner's, as stored */
  float pos_img[2];     /* winner's, as stored */
} rebvio_hip_kf_match;
int rebvio_hip_map_keyframe_matches(rebvio_hip_map* map, int kf_size, rebvio_hip_kf_match* out_host, int cap, int* count);

/* Keyframe snapshot. A map that serves as a pair's old map is rotated in place, pair after pair, so the keyframe's keylines in the
 * keyframe's OWN camera frame are gone once tracking has moved on. A snapshot keeps them: pos_img, (rho, sigma_rho) and matches of
 * every keyline i < size, and the size, copied by one kernel into buffers the handle owns (16 bytes + 4 bytes per keyline).
 * rebvio_hip_map_keyframe_snapshot queues that kernel on the TRACK stream in call order and waits for nothing on the host, as
 * rebvio_hip_map_mark_keyframe does, and follows its calling rules. The snapshot holds the keylines as they are when the kernel runs
 * in stream order: take it where the mark is made, after the map has been a pair's new map and before it serves as an old one. A
 * map promised to R_prior_next is already rotated for the next pair and is refused (-7), like its cloud. -3, before the device is
 * touched: null context, map or output, a map of another context; -10: the context has been destroyed.
 * rebvio_hip_kf_snapshot_download (synchronous, track-side): *n = the keyframe's size; min(n, cap) records of prs4 = (pos_img.x,
 * pos_img.y, rho, sigma_rho) and of matches are written (either may be NULL with cap 0). -3: null snapshot or n, negative cap, a
 * null buffer with cap > 0; -10: the context has been destroyed.
 * rebvio_hip_kf_snapshot_release: exactly once per handle; safe after rebvio_hip_destroy (which frees the buffers). */
typedef struct rebvio_hip_kf_snapshot rebvio_hip_kf_snapshot;
int rebvio_hip_map_keyframe_snapshot(rebvio_hip_ctx* ctx, rebvio_hip_map* map, rebvio_hip_kf_snapshot** out);
void rebvio_hip_kf_snapshot_release(rebvio_hip_kf_snapshot* snap);
int rebvio_hip_kf_snapshot_download(rebvio_hip_kf_snapshot* snap, float* prs4, unsigned* matches, int cap, int* n);

/* Pose of a map relative to its keyframe, X_cur = R X_kf + t in keyframe depth units (a keyframe keyline of inverse depth rho lies
 * at depth 1 / rho, as in a cloud of scale 1), estimated on the device from the keyframe correspondences by Gauss-Newton on the
 * edge-normal reprojection error with Huber weights; fp64 from the loads on, every + - * / and sqrt one IEEE operation, in the
 * order written here.
 * Candidates: the records of rebvio_hip_map_keyframe_matches(map, kf_size = the snapshot's size), left in device memory;
 * `candidates` is their number. For a record (j = kf_keyline, i = keyline), with fm of the context's parameters, pos_img_j, rho_j,
 * sigma_rho_j, matches_j of the snapshot and pos_img_i, gradient_i = (gx, gy) of the map:
 *   a = (double)(pos_img_j.x / fm);  b = (double)(pos_img_j.y / fm);  rho = (double)rho_j       (fp32 divisions, as rotateKeylines)
 *   q.x = (double)(pos_img_i.x / fm);  q.y = (double)(pos_img_i.y / fm)
 *   g2 = gx * gx + gy * gy;  gn = sqrt(g2);  n.x = gx / gn;  n.y = gy / gn
 *   Z[r] = (R[3r] * a + R[3r+1] * b) + R[3r+2];  Y[r] = Z[r] + rho * t[r]                       (r = 0, 1, 2 = x, y, z)
 *   p.x = Y.x / Y.z;  p.y = Y.y / Y.z;  e = fm * (n.x * (p.x - q.x) + n.y * (p.y - q.y))        (pixels along the gradient)
 *   c.x = (fm * n.x) / Y.z;  c.y = (fm * n.y) / Y.z;  c.z = -(c.x * p.x + c.y * p.y)
 *   J = (rho * c.x, rho * c.y, rho * c.z,  Z.y * c.z - Z.z * c.y,  Z.z * c.x - Z.x * c.z,  Z.x * c.y - Z.y * c.x)
 *       (the derivative of e for t <- t + dt, R <- exp(dw) R)
 *   |e| <= huber_px:  w = 1, cost = (e * e) / 2;   otherwise  w = huber_px / |e|, cost = huber_px * (|e| - huber_px / 2)
 * The term is used when ALL of these hold (positive tests: a NaN skips it): keyframe keyline j passes kf_filter (matches_j >=
 * min_matches, rho_j >= rho_min, rho_j <= rho_max, sigma_rho_j <= max_rel_sigma * rho_j in fp32, the point cloud's test); g2 > 0 and
 * g2 < infinity; Y.z > 0. The 28 sums over the used terms: (w * J[a]) * J[b] for a <= b (H, returned as the full symmetric 6x6,
 * row-major), (w * J[a]) * e (g), cost; `used` counts the terms. Summation order: the 64 lanes of a wave by a butterfly (lane l
 * adds lane l ^ 32, then ^ 16, ... ^ 1), the four waves of a workgroup of 256 records as (w0 + w1) + (w2 + w3), the workgroups in
 * ascending order from 0.0 - a fixed tree and no floating-point atomic: the same bits on every run.
 * One evaluation = these sums at the current pose. Behind every evaluation but the last, H d = -g is solved by Cholesky (H = L L',
 * column by column; forward, then back substitution) and t[r] += d[r], R = E R with w = d[3..5], th2 = (w.x * w.x + w.y * w.y) +
 * w.z * w.z, K = [w]x, E = (I + A K) + B (K K), A = sin(th) / th, B = (1 - cos(th)) / th2, th = sqrt(th2) - and A = 1, B = 0
 * when th2 < 1e-16. max_iter + 1 evaluations are queued back to back on the track stream (2 * max_iter + 2 launches behind the
 * three of the correspondences), with no host wait in between and no early exit; the result is copied once. H, g, cost and used
 * are those of the LAST evaluation, i.e. at the returned pose; iterations = steps applied.
 * status 0: ok. 3: used < min_used at the first evaluation; 2: a pivot of the factorisation was not > 0 or not finite. In both
 * cases the pose stays what it was at that point (3: the guess) and the remaining steps change nothing. max_iter 0 evaluates the
 * sums at the guess only. A snapshot of size 0: candidates 0, used 0, status 3, pose = guess, zero sums; no kernel is launched.
 * Synchronous and track-side with the calling rules of rebvio_hip_map_keyframe_matches; the map counts as used by the tracker
 * afterwards. -3, before the device is touched: null map, snapshot or output, a non-finite R0 or t0, an invalid kf_filter (the
 * point cloud's rules), huber_px not > 0, max_iter outside 0..32, min_used outside 0..65536, a snapshot of another context;
 * -10: the context has been destroyed; -7: the map is promised to R_prior_next.
 * rebvio_hip_test_kf_pose_host (test hook, touches no device) runs the same statements on the host from caller arrays - the
 * snapshot's prs4 / matches (kf_size keyframe keylines), the current map's pos_img / gradient (n_cur x 2 floats each), n_rec
 * candidate records of which kf_keyline and keyline are read - and sums the terms in record order. -3: a null array, a record
 * whose indices lie outside the arrays, or options / a guess the device entry refuses. */
typedef struct rebvio_hip_kf_pose_opts { /* defaults from rebvio_hip_default_kf_pose_opts */
  rebvio_hip_cloud_filter kf_filter;     /* applied to the KEYFRAME side of a correspondence; default = default cloud filter */
  double huber_px;                       /* default 2.0 */
  int max_iter;                          /* 0..32, default 8; 0 = evaluate the sums at the guess only */
  int min_used;                          /* default 12 */
} rebvio_hip_kf_pose_opts;
typedef struct rebvio_hip_kf_pose {
  double R[9], t[3];                     /* X_cur = R X_kf + t, keyframe depth units (1/rho, as a cloud of scale 1) */
  double H[36], g[6], cost;              /* sums at the RETURNED pose: J^T W J, J^T W e, sum of Huber costs */
  int candidates, used, iterations, status; /* status 0 ok, 2 H not positive definite, 3 used < min_used at the first evaluation */
} rebvio_hip_kf_pose;
void rebvio_hip_default_kf_pose_opts(rebvio_hip_kf_pose_opts* opts);
int rebvio_hip_map_keyframe_pose(rebvio_hip_map* map, rebvio_hip_kf_snapshot* snap, const rebvio_hip_kf_pose_opts* opts,
                                 const double R0[9] /*NULL = identity*/, const double t0[3] /*NULL = 0*/, rebvio_hip_kf_pose* out);
int rebvio_hip_test_kf_pose_host(float fm, const float* snap_prs4, const unsigned* snap_matches, int kf_size, const float* cur_pos_img,
                                 const float* cur_gradient, int n_cur, const rebvio_hip_kf_match* records, int n_rec,
                                 const rebvio_hip_kf_pose_opts* opts, const double R0[9], const double t0[3], rebvio_hip_kf_pose* out);

/* Normals for a snapshot. rebvio_hip_kf_snapshot_add_normals queues one kernel (k_kf_snapshot_normals, one workgroup of 256 per 256
 * keylines, both sizes read on the device) on the TRACK stream in call order and waits for nothing on the host: for
 * i < min(map size, snapshot size)  n_i = (gradient_i.x / gradient_norm_i, gradient_i.y / gradient_norm_i), two fp32 IEEE divisions,
 * and (0, 0) for every other slot and wherever gradient_norm_i is not > 0. The first call gives the snapshot one more device buffer
 * (8 bytes per slot, one more live resource, freed with the snapshot or its context); a later call overwrites it. The calling rules
 * are the snapshot's: take the normals where the mark and the snapshot are taken, from the map the snapshot was taken from (the
 * caller's contract). -7: the map is promised to R_prior_next (its gradients are already rotated); -3, before the device is touched:
 * null snapshot or map, a map of another context; -10: the context has been destroyed.
 * rebvio_hip_kf_snapshot_download_normals (synchronous, track-side): *n = the snapshot's size, min(n, cap) pairs written to n2.
 * -7: no normals were added; -3: null snapshot or n, negative cap, null n2 with cap > 0; -10. */
int rebvio_hip_kf_snapshot_add_normals(rebvio_hip_kf_snapshot* snap, rebvio_hip_map* map);
int rebvio_hip_kf_snapshot_download_normals(rebvio_hip_kf_snapshot* snap, float* n2, int cap, int* n);

/* Alignment of a keyframe snapshot to a map through the map's distance field: the pose X_cur = R X_kf + t of
 * rebvio_hip_map_keyframe_pose, but with the associations found as Core::tryVel finds them (rebvio/src/core.cpp) - a keyframe keyline
 * is projected under the current pose and takes the keyline of the map that owns the cell it lands in - instead of the
 * match_id_keyframe chain. Only the map's distance field, pos and gradient / gradient_norm as DistanceField::build formed it are
 * read: tracking never writes them, so any detected map of the snapshot's context can be aligned at any time, a map promised to
 * R_prior_next included. fp64 behind the loads, every + - * / sqrt and floor one IEEE operation in the order written here.
 * One term per keyframe keyline j < size (`candidates` = the snapshot's size), with fm, cx, cy, rows, cols, search_range of the
 * context, (R, t) the current pose and pos_img_j, rho_j, sigma_rho_j, matches_j, and the normal (nx_j, ny_j) where normals were
 * added, of the snapshot. The term is used when ALL of these hold (positive tests: a NaN skips it):
 *   1. keyframe keyline j passes kf_filter (the test of rebvio_hip_map_keyframe_pose).
 *   2. a, b, rho, Z, Y as in rebvio_hip_map_keyframe_pose;  Y.z > 0.
 *   3. p.x = Y.x / Y.z;  p.y = Y.y / Y.z;  u = (double)fm * p.x + (double)cx;  v = (double)fm * p.y + (double)cy;
 *      x = floor(u + 0.5);  y = floor(v + 0.5);  1 <= x <= cols - 2  and  1 <= y <= rows - 2  (tested in double, before any conversion).
 *   4. key = df[y * cols + x] is not empty; i = the owning keyline and dist = its distance in cells, as rebvio_hip_map_distance_field
 *      reports them; dist <= max_dist.
 *   5. n_i = unit_i (the map's gradient_i / gradient_norm_i as the field was built from). Where the snapshot has normals and
 *      min_cos > -1:  m.x = R[0] * nx_j + R[1] * ny_j;  m.y = R[3] * nx_j + R[4] * ny_j;  mm = m.x * m.x + m.y * m.y;
 *      nn = n_i.x * n_i.x + n_i.y * n_i.y;  when mm > 0 and nn > 0:  m.x * n_i.x + m.y * n_i.y >= (min_cos * sqrt(mm)) * sqrt(nn).
 *      Otherwise (no normals, min_cos == -1, a zero normal on either side) no gate is applied.
 *   6. q.x = pos_i.x - cx;  q.y = pos_i.y - cy  (fp32 subtractions); then the term of rebvio_hip_map_keyframe_pose with q for
 *      pos_img_i and n_i for gradient_i, with its own skips (g2 > 0 and < infinity, Y.z > 0).
 * assoc[j] = i when the term is used, -1 otherwise; every evaluation writes all of it, and assoc_host (NULL, or room for the
 * snapshot's size) gets the last evaluation's, i.e. the associations at the returned pose.
 * The 28 sums, their summation tree (one thread per keyframe keyline, workgroups of 256), the Gauss-Newton step, status 0 / 2 / 3,
 * H, g, cost, used and iterations are those of rebvio_hip_map_keyframe_pose: max_iter + 1 evaluations queued back to back,
 * 2 * max_iter + 2 launches (none for correspondences), no host wait in between and no early exit. The associations change from
 * evaluation to evaluation; used is tested against min_used at the first one only, and a later H that does not factor gives 2.
 * A snapshot of size 0: status 3, pose = guess, nothing launched.
 * Synchronous and track-side; the map counts as used by the tracker afterwards; the context's scratch (one allocation) is made at
 * the first call. -3, before the device is touched: null map, snapshot or output, a non-finite R0 or t0, an invalid kf_filter,
 * huber_px not > 0, min_cos outside [-1, 1] or NaN, max_dist outside 0..search_range, max_iter outside 0..32, min_used outside
 * 0..65536, a snapshot of another context; -10: the context has been destroyed; -7: the map's field is not detection's (none built,
 * or the keylines were uploaded: unit is detection's).
 * rebvio_hip_test_kf_align_host (test hook, touches no device) runs the same statements on the host from caller arrays - the
 * camera, the snapshot's prs4 / matches and normals (or NULL) for kf_size keyframe keylines, the map's pos and unit (n_cur x 2 floats
 * each), the field as rebvio_hip_map_distance_field returns it (rows * cols ids, -1 = empty, and distances) - and sums the terms in
 * index order; opts NULL = the defaults with max_dist = search_range (opts->max_dist is tested against search_range). -3: a null
 * array, a field id outside the keyline arrays, or options / a guess the device entry refuses. */
typedef struct rebvio_hip_kf_align_opts { /* defaults from rebvio_hip_default_kf_align_opts */
  rebvio_hip_cloud_filter kf_filter;     /* keyframe side, as in rebvio_hip_kf_pose_opts */
  double huber_px;                       /* default 2.0 */
  double min_cos;                        /* default 0.9; used only where the snapshot has a non-zero normal; -1 disables */
  int max_dist;                          /* 0..search_range cells; default = the context's search_range (no gate) */
  int max_iter, min_used;                /* as rebvio_hip_kf_pose_opts: 0..32 default 8; 0..65536 default 12 */
} rebvio_hip_kf_align_opts;
void rebvio_hip_default_kf_align_opts(rebvio_hip_ctx* ctx /*NULL: max_dist = 40, the default search_range*/, rebvio_hip_kf_align_opts* opts);
int rebvio_hip_map_keyframe_align(rebvio_hip_map* map, rebvio_hip_kf_snapshot* snap, const rebvio_hip_kf_align_opts* opts,
                                  const double R0[9] /*NULL = identity*/, const double t0[3] /*NULL = 0*/, rebvio_hip_kf_pose* out,
                                  int* assoc_host /*NULL or snapshot-size ints*/);
int rebvio_hip_test_kf_align_host(float fm, float cx, float cy, int rows, int cols, int search_range, const float* snap_prs4,
                                  const unsigned* snap_matches, const float* snap_normals /*NULL: none*/, int kf_size,
                                  const float* cur_pos, const float* cur_unit, int n_cur, const int* df_id, const int* df_dist,
                                  const rebvio_hip_kf_align_opts* opts, const double R0[9], const double t0[3], rebvio_hip_kf_pose* out,
                                  int* assoc /*NULL or kf_size ints*/);

/* Many hypotheses against one map in one set of launches. A hypothesis is a snapshot and a guess (R0, t0); for every h < n,
 * out[h].pose is BIT FOR BIT what rebvio_hip_map_keyframe_align(map, hyp[h].snap, opts, hyp[h].R0, hyp[h].t0, &p, NULL) returns for
 * the same arguments - every field, status 2 and 3 included: the per-keyline statement, the summation tree and the step are that
 * entry's, and a hypothesis's sums never meet another's. One options block (NULL = the defaults) serves all hypotheses. The same
 * snapshot may appear any number of times (several starts around one guess), snapshots with and without normals may be mixed, and
 * a snapshot of size 0 behaves as it does there (status 3, pose = guess, zero sums, inliers 0 - for min_used 0 too).
 * inliers = the number of used terms with |e| <= huber_px (the first branch of the Huber test) at the evaluation whose H, g, cost
 * and used the result carries; an integer count. There is NO assoc output: a caller that wants the winner's associations runs
 * rebvio_hip_map_keyframe_align on it, from the guess (the same pose, bit for bit) or from the returned pose with max_iter 0.
 * Launches: max_iter + 1 evaluations of two kernels each, 2 * max_iter + 2 on the track stream WHATEVER n is - k_kf_align_sums_many
 * over a grid of (the largest ceil(size / 256) of the list, n) workgroups of 256, where a workgroup behind its own hypothesis's last
 * keyline leaves at once, and k_kf_pose_step_many, one workgroup of 64 per hypothesis. In front of them ONE upload (the table of n
 * descriptors and the n start states), behind them ONE copy of the n results; no host wait in between, no early exit. A list whose
 * snapshots are all of size 0 launches nothing. Synchronous and track-side under the calling rules of rebvio_hip_map_keyframe_align;
 * the map counts as used by the tracker afterwards. The context's scratch for this entry (one allocation, one more live resource:
 * REBVIO_HIP_KF_HYP_MAX x (descriptor + result block + 256 partials of 28 doubles + 256 used counts + 256 inlier counts)) is made at the
 * first call that reaches the device and kept.
 * -3, before the device is touched: null map, hyp or out; n outside 1..REBVIO_HIP_KF_HYP_MAX; a null snapshot; a snapshot of another
 * context; a non-finite guess; options rebvio_hip_map_keyframe_align refuses. -10 and -7: exactly as that entry.
 * rebvio_hip_kf_align_best (host only, a pure function): the index of the best result among those with pose.status == 0 and
 * inliers >= min_inliers - the most inliers, then the smaller pose.cost, then the lower index; -1 when none qualifies; -3: null
 * array or n < 1.
 * rebvio_hip_kf_hypotheses_around (host only, touches no device): 13 starts around (R, t) for `snap` (stored as given, may be NULL).
 * out[0] = (R, t) exactly. out[1 + 2a + s], a = 0, 1, 2, s = 0, 1: R <- E R with w = (s ? -rot_step : +rot_step) e_a and the
 * E = (I + A K) + B (K K) of the Gauss-Newton step above (its statements, in fp64), t unchanged. out[7 + 2a + s]: t[a] + trans_step
 * (s = 0) or t[a] - trans_step (s = 1), R unchanged. -3: null R, t or out, a non-finite R, t or step, a negative step.
 * rebvio_hip_test_kf_align_many_host (test hook, touches no device): rebvio_hip_test_kf_align_host's statements for n guesses
 * R0s[9 n], t0s[3 n] against ONE snapshot's arrays; out[h].pose is that hook's result byte for byte, out[h].inliers the count above
 * from the same term values. -3: what that hook refuses, a null R0s, t0s or out, n outside 1..REBVIO_HIP_KF_HYP_MAX. */
#define REBVIO_HIP_KF_HYP_MAX 64
typedef struct rebvio_hip_kf_hypothesis { /* 104 bytes */
  rebvio_hip_kf_snapshot* snap;
  double R0[9], t0[3];                   /* the guess: X_cur = R0 X_kf + t0 */
} rebvio_hip_kf_hypothesis;
typedef struct rebvio_hip_kf_hyp_result { /* sizeof(rebvio_hip_kf_pose) + 8 */
  rebvio_hip_kf_pose pose;
  int inliers;                           /* used terms with |e| <= huber_px at the returned pose */
  int reserved;                          /* 0 */
} rebvio_hip_kf_hyp_result;
int rebvio_hip_map_keyframe_align_many(rebvio_hip_map* map, const rebvio_hip_kf_hypothesis* hyp, int n,
                                       const rebvio_hip_kf_align_opts* opts, rebvio_hip_kf_hyp_result* out /* n */);
int rebvio_hip_kf_align_best(const rebvio_hip_kf_hyp_result* res, int n, int min_inliers);
int rebvio_hip_kf_hypotheses_around(rebvio_hip_kf_snapshot* snap, const double R[9], const double t[3], double rot_step,
                                    double trans_step, rebvio_hip_kf_hypothesis out[13]);
int rebvio_hip_test_kf_align_many_host(float fm, float cx, float cy, int rows, int cols, int search_range, const float* snap_prs4,
                                       const unsigned* snap_matches, const float* snap_normals /*NULL: none*/, int kf_size,
                                       const float* cur_pos, const float* cur_unit, int n_cur, const int* df_id, const int* df_dist,
                                       const rebvio_hip_kf_align_opts* opts, const double* R0s /*9 n*/, const double* t0s /*3 n*/, int n,
                                       rebvio_hip_kf_hyp_result* out /* n */);

/* Depth fusion into a keyframe snapshot: every map aligned to a snapshot is a new view of the keyframe's edges from a known pose,
 * and rebvio_hip_kf_snapshot_fuse_depth folds that view into the snapshot's rho / sigma_rho with one scalar Kalman update per
 * associated keyline, as Core::updateInverseDepth does per pair (rebvio/src/core.cpp) - without its propagation and rescaling,
 * since the keyframe's frame does not move. The measurement is the pixel position of the map's keyline along its gradient, never
 * the map's rho (which descends from the keyframe's own through the forward matches). (R, t) is the pose X_cur = R X_kf + t, e.g.
 * the one rebvio_hip_map_keyframe_align returned. Fusing the same map twice counts its pixels twice: the caller's contract.
 * fp64 behind the loads, every + - * / and sqrt one IEEE operation in the order written. Per keyframe keyline j < size:
 *   1. steps 1..6 of rebvio_hip_map_keyframe_align at (R, t), with kf_filter, min_cos and max_dist of these options, give the owner
 *      i - or the keyline is not associated.
 *   2. e, c.x, c.y, c.z of the term of rebvio_hip_map_keyframe_pose; no Huber weight.
 *   3. h = (c.x * t[0] + c.y * t[1]) + c.z * t[2]                  (de/drho, since dY/drho = t)
 *   4. s = (double)sigma_rho_j;  v = s * s + q_abs * q_abs;  hv = h * v;  info = hv * h;   flat unless info > 0.
 *   5. S = info + pixel_sigma * pixel_sigma;   gated unless e * e <= (gate_sigma * gate_sigma) * S.
 *   6. K = hv / S;  rho_n = rho - K * e;  v_n = (1.0 - K * h) * v;  sig_n = sqrt(v_n);   gated unless rho_n, v_n and sig_n are
 *      finite and v_n >= 0 (positive tests: a NaN gates).
 *   7. rho_n < RHO_MIN:  sig_n = sig_n + (RHO_MIN - rho_n);  rho_n = RHO_MIN;   else rho_n > RHO_MAX:  rho_n = RHO_MAX;   either
 *      counts as clamped. RHO_MIN = (double)1e-3f and RHO_MAX = 20 are what the tracker clamps to.
 *   8. the snapshot gets (float)rho_n, (float)sig_n and matches_j + 1 (saturating at 0xFFFFFFFF). pos_img and the normals are never
 *      written; a keyline that is not fused keeps all its bits.
 * assoc[j] = i when fused, -1 - i when gated or flat, INT_MIN when not associated. associated = fused + gated + flat.
 * One kernel (k_kf_fuse_depth: one thread per keyframe keyline, workgroups of 256, at most 256 of them with a stride loop behind;
 * sizes read on the device), one clear of the count block and one copy back; the counts are integer sums, no floating-point value
 * crosses threads: every output word is the same on every run. Synchronous and track-side; map acceptance as
 * rebvio_hip_map_keyframe_align (any detected map of the snapshot's context, promised or not; -7 where the field is not
 * detection's). The first call gives the context one more device allocation (the counts and keylines_max association words: one
 * more live resource, kept until the context goes). A snapshot of size 0: all counts zero, nothing launched or allocated.
 * -3, before the device is touched: null snapshot, map, R, t or output, a non-finite R or t, an invalid kf_filter, pixel_sigma or
 * gate_sigma not > 0, q_abs < 0 or NaN, min_cos outside [-1, 1], max_dist outside 0..search_range, reserved != 0, a snapshot of
 * another context; -10: the context has been destroyed. opts NULL = the defaults.
 * rebvio_hip_test_kf_fuse_host (test hook, touches no device): the same statements on the host over the arrays of
 * rebvio_hip_test_kf_align_host, snap_prs4 and snap_matches updated in place; opts NULL = the defaults with max_dist = search_range. */
typedef struct rebvio_hip_kf_fuse_opts {   /* defaults from rebvio_hip_default_kf_fuse_opts */
  rebvio_hip_cloud_filter kf_filter;       /* keyframe side, as in rebvio_hip_kf_align_opts; default = default cloud filter */
  double min_cos;                          /* as in rebvio_hip_kf_align_opts, default 0.9 */
  double pixel_sigma;                      /* > 0; default = the context's pixel_uncertainty (NULL ctx: its default value) */
  double gate_sigma;                       /* > 0; default 3.0: innovation gate in standard deviations */
  double q_abs;                            /* >= 0; default 0: added in quadrature to sigma_rho before the update */
  int max_dist;                            /* 0..search_range, default search_range */
  int reserved;                            /* 0 */
} rebvio_hip_kf_fuse_opts;
typedef struct rebvio_hip_kf_fuse {
  int candidates;   /* the snapshot's size */
  int associated;   /* keylines that passed steps 1..6 of the alignment's definition */
  int fused;        /* ...and were updated */
  int gated;        /* ...failed the innovation gate or gave a non-finite update (left as they were) */
  int flat;         /* ...carried no information: !(h * v * h > 0) (left as they were) */
  int clamped;      /* among fused: rho ran into RHO_MIN or RHO_MAX */
} rebvio_hip_kf_fuse;
void rebvio_hip_default_kf_fuse_opts(rebvio_hip_ctx* ctx /*NULL: pixel_sigma = 1, max_dist = 40, the defaults*/, rebvio_hip_kf_fuse_opts* opts);
int rebvio_hip_kf_snapshot_fuse_depth(rebvio_hip_kf_snapshot* snap, rebvio_hip_map* map, const rebvio_hip_kf_fuse_opts* opts,
                                      const double R[9], const double t[3], rebvio_hip_kf_fuse* out,
                                      int* assoc_host /*NULL or snapshot-size ints*/);
int rebvio_hip_test_kf_fuse_host(float fm, float cx, float cy, int rows, int cols, int search_range, float* snap_prs4 /*in/out*/,
                                 unsigned* snap_matches /*in/out*/, const float* snap_normals /*NULL: none*/, int kf_size,
                                 const float* cur_pos, const float* cur_unit, int n_cur, const int* df_id, const int* df_dist,
                                 const rebvio_hip_kf_fuse_opts* opts, const double R[9], const double t[3], rebvio_hip_kf_fuse* out,
                                 int* assoc /*NULL or kf_size ints*/);

/* Depth prior from a registered depth image (RGB-D): rebvio_hip_map_fuse_depth_image folds a sensor's depth for frame k into the
 * (rho, sigma_rho) of map k's keylines with one scalar Kalman update per keyline - the input side of the depth-bearing products
 * above. No reference counterpart. Without it a keyline starts at rho = 1, sigma_rho = 20 and earns its depth from motion alone, in
 * an arbitrary scale; with it the map's depths, and V, are metric.
 * Geometry: the image has the context's rows x cols and lies in the geometry of the image the detector sees (with a lens model:
 * behind the front end's undistortion; resampling a raw depth image is the caller's). It holds the depth along the optical axis.
 * Formats: REBVIO_HIP_DEPTH_U16, z = value * unit (unit: metres per count, default 0.001), a value of 0 is invalid;
 * REBVIO_HIP_DEPTH_F32, z = value in metres. Rows are pitch_bytes apart (0 = dense; otherwise >= cols * the tap's size and a
 * multiple of it; the image starts aligned to the tap's size). A tap's depth is valid when z_min <= z && z <= z_max (positive
 * tests: a NaN fails them).
 * fp64 behind the loads; every + - * / sqrt and floor one IEEE operation in the order written, no contraction. Per keyline i < size:
 *   1. px = pos[0], py = pos[1] - the detector's pixel position, NOT pos_img, which earlier pairs may have rotated.
 *      The direction is usable when gradient_norm > 0 and ux = gradient[0] / gradient_norm, uy = gradient[1] / gradient_norm are
 *      both finite.
 *   2. The centre tap is at (x, y) = (px, py). With a usable direction two side taps, s = +1 then s = -1:  d = s * tap_px;
 *      x = px + d * ux;  y = py + d * uy.  A tap is inside when x + 0.5 >= 0 && x + 0.5 < cols && y + 0.5 >= 0 && y + 0.5 < rows
 *      (a NaN or infinite position is outside); then xi = (int)floor(x + 0.5), yi = (int)floor(y + 0.5) and the tap reads the image
 *      at row yi, column xi. z_near = the minimum, z_far = the maximum of the valid taps' z. No valid tap: NO DEPTH, the keyline
 *      keeps all its bits. jump: z_far - z_near > jump_rel * z_near (an edge is often an occlusion boundary; the nearer surface
 *      owns an occluding edge, so the measurement is z_near either way).
 *   3. rho_m = 1.0 / z_near;  s_m = (sigma_z0 * rho_m) * rho_m + sigma_z2   (a sensor with sigma_z = sigma_z0 + sigma_z2 * z^2,
 *      carried to inverse depth).
 *   4. s = (double)sigma_rho;  v = s * s + q_abs * q_abs;  e = rho_m - (double)rho;  S = v + s_m * s_m;
 *      GATED, the keyline left as it was, unless e * e <= (gate_sigma * gate_sigma) * S.
 *   5. K = v / S;  rho_n = rho + K * e;  v_n = (1.0 - K) * v;  sig_n = sqrt(v_n);  also GATED unless rho_n, v_n and sig_n are finite
 *      and v_n >= 0 (positive tests). Then step 7 of rebvio_hip_kf_snapshot_fuse_depth: the RHO_MIN / RHO_MAX clamp, counted as clamped.
 *   6. FUSED: the map gets (float)rho_n and (float)sig_n. matches and every other field are untouched: a sensor depth is not a
 *      tracking match.
 * outcome[i] = 0 no depth, 1 fused, 2 gated;  + 16 for a jump (with 1 or 2),  + 32 for clamped (with 1). Counts: candidates = the
 * map's size, sampled = fused + gated, jumps among the sampled, clamped among the fused - integer sums; no floating-point value
 * crosses threads, every output word is the same on every run.
 * Where in a stream: the image of frame k goes into map k AFTER the pair in which k was the new map (directedMatch overwrites a
 * matched new keyline's depth) - or right after detection for a stream's first map - and BEFORE map k serves as an old map.
 * Map acceptance: -7 for a map promised to R_prior_next (already rotated for the next pair, like its cloud) and for a map that has
 * served as the old map of rebvio_hip_track_pair / rebvio_hip_track_pair_begin (its rho lives in a newer frame); -10: the context
 * has been destroyed; -3, before the device is touched: a null map, image or counts, an unknown format, a bad pitch or alignment,
 * a map of another context, an invalid option (rebvio_hip_last_error names it).
 * One kernel per call (k_depth_prior: one thread per keyline, ceil(keylines_max / 256) workgroups of 256, the size read on the
 * device) behind one clear of the count block, all on the TRACK stream; the entries follow the track-side thread rule of
 * rebvio_hip_map_point_cloud, and the map counts as used by the tracker afterwards. The first call gives the context one more owned
 * device allocation (the counts and keylines_max outcome words: one more live resource, kept until the context goes); the first
 * call of the HOST-image entry one pinned staging frame of its own besides (the detect entries' ring belongs to the detect-side
 * thread). A map of size 0: all counts zero.
 *   rebvio_hip_map_fuse_depth_image         host image, copied into the pinned staging frame, which the kernel reads in place;
 *                                           synchronous. outcome_host: NULL, or room for the map's size.
 *   rebvio_hip_map_fuse_depth_image_device  the same for an image in device memory; synchronous.
 *   rebvio_hip_map_fuse_depth_image_async   device image; queued in call order, returns at once - for use between _finish_async(k)
 *                                           and _begin(k+1). The image must stay unchanged until the kernel has run. The counts stay
 *                                           in device memory: rebvio_hip_depth_prior_last_counts fetches those of the context's most
 *                                           recent fusion (any entry) and waits for them; all zero before the first.
 *   rebvio_hip_test_depth_prior_host        test hook, touches no device: the same statements over n keylines (rho / sigma_rho updated
 *                                           in place) in index order. -3 as above, and for a negative n or size. */
#define REBVIO_HIP_DEPTH_U16 0
#define REBVIO_HIP_DEPTH_F32 1
typedef struct rebvio_hip_depth_prior_opts { /* defaults from rebvio_hip_default_depth_prior_opts */
  double tap_px;     /* >= 0, default 2.0: distance of the side taps along the gradient, pixels */
  double jump_rel;   /* >= 0, default 0.1 */
  double z_min;      /* > 0, default 0.1 m */
  double z_max;      /* >= z_min, default 20 m */
  double sigma_z0;   /* >= 0, default 1e-3 m */
  double sigma_z2;   /* >= 0, default 2e-3 1/m; sigma_z0 + sigma_z2 > 0 */
  double gate_sigma; /* > 0, default 3.0: innovation gate in standard deviations */
  double q_abs;      /* >= 0, default 0: added in quadrature to sigma_rho before the update */
  double unit;       /* > 0, default 0.001: metres per count of a U16 image */
  int reserved;      /* 0 */
} rebvio_hip_depth_prior_opts;
typedef struct rebvio_hip_depth_prior_counts {
  int candidates; /* the map's size */
  int sampled;    /* keylines with at least one valid tap */
  int fused;      /* ...updated */
  int gated;      /* ...failed the innovation gate or gave a non-finite update (left as they were) */
  int jumps;      /* among sampled: z_far - z_near > jump_rel * z_near */
  int clamped;    /* among fused: rho ran into RHO_MIN or RHO_MAX */
} rebvio_hip_depth_prior_counts;
void rebvio_hip_default_depth_prior_opts(rebvio_hip_depth_prior_opts* opts);
int rebvio_hip_map_fuse_depth_image(rebvio_hip_map* map, const void* depth_host, size_t pitch_bytes, int fmt,
                                    const rebvio_hip_depth_prior_opts* opts /*NULL = defaults*/, rebvio_hip_depth_prior_counts* counts,
                                    int* outcome_host /*NULL ok*/);
int rebvio_hip_map_fuse_depth_image_device(rebvio_hip_map* map, const void* depth_dev, size_t pitch_bytes, int fmt,
                                           const rebvio_hip_depth_prior_opts* opts, rebvio_hip_depth_prior_counts* counts,
                                           int* outcome_host /*NULL ok*/);
int rebvio_hip_map_fuse_depth_image_async(rebvio_hip_ctx* ctx, rebvio_hip_map* map, const void* depth_dev, size_t pitch_bytes, int fmt,
                                          const rebvio_hip_depth_prior_opts* opts);
int rebvio_hip_depth_prior_last_counts(rebvio_hip_ctx* ctx, rebvio_hip_depth_prior_counts* counts);
int rebvio_hip_test_depth_prior_host(int rows, int cols, rebvio_hip_keyline* keylines /*in/out*/, int n, const void* depth,
                                     size_t pitch_bytes, int fmt, const rebvio_hip_depth_prior_opts* opts,
                                     rebvio_hip_depth_prior_counts* counts, int* outcome /*NULL or n ints*/);

/* Depth prior from a rectified stereo partner: rebvio_hip_map_fuse_stereo searches, for every keyline of the LEFT map, the edge map
 * detected in the RIGHT image of the same instant along the keyline's row, and folds the disparity it finds into the keyline's
 * (rho, sigma_rho) with one scalar Kalman update - inverse depth is linear in disparity, rho = d / (fm * baseline). No reference
 * counterpart. With it the map's depths, and V, are metric from the first frame on.
 * Geometry: the pair is rectified - both images have the left context's rows x cols, fm, cx, cy, rows are aligned, the right camera
 * sits at +baseline metres along the left camera's x axis: a point at depth z has disparity d = x_left - x_right = fm * baseline / z.
 * Rectifying rotations are the caller's, as the registration of a depth image is.
 * The left map is the tracker's. The right map is any detected map with the same rows and cols on the same device, of the left
 * context or of another live one (a second camera wants its own threshold servo: a second, detect-only context is the intended
 * source). It is only read.
 * fp64 behind the loads; every + - * / sqrt, floor and ceil one IEEE operation in the order written, no contraction; a / b / c and
 * a * b / c associate from the left. fb = (double)fm * baseline. Per left keyline i < size:
 *   1. px = pos[0], py = pos[1] - the detector's position, NOT pos_img (as in the depth prior). The direction is usable when
 *      gradient_norm > 0, ux = gradient[0] / gradient_norm and uy = gradient[1] / gradient_norm are both finite and
 *      fabs(ux) >= min_ux (an edge parallel to the epipolar line measures no disparity). Otherwise UNUSABLE, all bits kept.
 *   2. Inside means px + 0.5 >= 0 && px + 0.5 < cols && py + 0.5 >= 0 && py + 0.5 < rows (a NaN or infinite position is outside):
 *      otherwise NONE. xi = (int)floor(px + 0.5), yi = (int)floor(py + 0.5). The window's rows are yi, and with row_tol = 1 also
 *      yi - 1 and yi + 1; its columns xi - (int)ceil(d_max) - 1 ... xi - (int)floor(d_min) + 1; both clipped to the image. The
 *      integer window is part of the definition.
 *   3. Per cell of the window with j = mask_right[cell], 0 <= j < the right map's size, (qx, qy) = pos, (hx, hy) = gradient and
 *      hn = gradient_norm of right keyline j: the keyline is a candidate when, in this order, hn > 0;
 *      (gx * hx + gy * hy) / (gn * hn) >= cos_min;  fabs(hn / gn - 1.0) <= norm_tol;  with uxr = hx / hn, uyr = hy / hn:
 *      fabs(uxr) >= min_ux;  xr = qx - (uyr * (py - qy)) / uxr  (where the right edge's tangent crosses the left keyline's row);
 *      d = px - xr;  d > 0 && d_min <= d && d <= d_max. All tests are positive: a NaN fails. A keyline with a candidate is SEEN;
 *      without one: NONE.
 *   4. rho_m = d / fb;  s_m = (sigma_px / fabs(ux)) / fb;  s = (double)sigma_rho;  v = s * s + q_abs * q_abs;  S = v + s_m * s_m;
 *      e = rho_m - (double)rho.  A candidate is IN the gate when e * e <= (gate_sigma * gate_sigma) * S. SEEN with none in: GATED.
 *   5. d_lo, d_hi = the smallest and the largest d of the candidates in the gate. d_hi - d_lo > ambig_px: AMBIGUOUS, the keyline is
 *      left as it was - its own prior is what disambiguates repeated structure once it is metric; a fresh keyline in front of a
 *      grating stays untouched.
 *   6. The winner is the candidate in the gate with the smallest (gx - hx) * (gx - hx) + (gy - hy) * (gy - hy), ties to the smaller
 *      j. With its d:  K = v / S;  rho_n = rho + K * e;  v_n = (1.0 - K) * v;  sig_n = sqrt(v_n);  GATED unless rho_n, v_n and
 *      sig_n are finite and v_n >= 0; then the RHO_MIN / RHO_MAX clamp of the depth prior's step 5, counted as clamped. FUSED: the
 *      map gets (float)rho_n and (float)sig_n. matches and every other field are untouched.
 * outcome[i] = 0 none, 1 fused, 2 gated, 3 unusable, 4 ambiguous;  + 32 for clamped (with 1). winner[i] = the winner's j where
 * fused, else -1. Counts: candidates = the left map's size, usable = those not UNUSABLE, seen, fused, gated, ambiguous, clamped -
 * integer sums. Only minima, maxima, an OR and integer sums cross threads: every output word is the same on every run and in any
 * order of the window's cells.
 * Where in a stream: as the depth image - the right map of frame k goes into left map k AFTER the pair in which k was the new map,
 * or right after detection for a stream's first map, and BEFORE map k serves as an old map. With a depth image for the same frame
 * the depth image goes first.
 * Map acceptance: the left map as for the depth image (-7 when promised to R_prior_next or when it has served as an old map; -10
 * when its context is destroyed). The right map: -3 when it is null, of another rows x cols or of another device; -10 when its
 * context is destroyed. -3 also for null counts, a left map of another context than ctx (queued entry) and an invalid option
 * (rebvio_hip_last_error names it); every -3 is checked before the device is touched.
 * One kernel per call (k_stereo_prior: 16 lanes per left keyline take consecutive cells of the window's rows, ceil(keylines_max /
 * 16) workgroups of 256, both sizes read on the device) behind one clear of the count block, on the LEFT context's track stream
 * under the track-side thread rule of rebvio_hip_map_point_cloud. Before queuing, the entry waits on the host for the right map's
 * own detection (as rebvio_hip_map_download of a fresh map does); what the right map's context has queued for it beyond that is
 * the caller's to order. The first call gives the left context one more owned device allocation (8 count words and 2 *
 * keylines_max words; kept until the context goes).
 *   rebvio_hip_map_fuse_stereo            synchronous. outcome_host, winner_host: NULL, or room for the left map's size each.
 *   rebvio_hip_map_fuse_stereo_async      queued in call order, returns at once - for use between _finish_async(k) and _begin(k+1).
 *                                         The caller keeps the right map unreleased until the counts have been fetched
 *                                         (rebvio_hip_stereo_prior_last_counts) or a later synchronising call on the left context
 *                                         has returned.
 *   rebvio_hip_stereo_prior_last_counts   the counts of ctx's most recent stereo fusion (either entry); waits for them; all zero
 *                                         before the first.
 *   rebvio_hip_test_stereo_prior_host     test hook, touches no device: the same statements over n left keylines (rho / sigma_rho
 *                                         updated in place) in index order, the window's cells row by row. right_mask: rows * cols
 *                                         ints; words outside [0, nr) are no keyline. -3 as above, and for a negative size. */
typedef struct rebvio_hip_stereo_prior_opts { /* defaults from rebvio_hip_default_stereo_prior_opts */
  double baseline;   /* > 0, no default (0 after the defaults call): metres between the cameras */
  double d_min;      /* default 0;  0 <= d_min <= d_max <= cols: accepted disparities, pixels */
  double d_max;      /* default 64 */
  double min_ux;     /* in (0, 1], default 0.5: least |x component| of a unit gradient, left and right */
  int row_tol;       /* 0 or 1, default 1: rows searched above and below the keyline's */
  double sigma_px;  /* > 0, default 0.5: standard deviation of a disparity along the gradient, pixels */
  double gate_sigma; /* > 0, default 3.0: innovation gate in standard deviations */
  double ambig_px;   /* >= 0, default 2.0: largest spread of the disparities in the gate */
  double cos_min;    /* in [-1, 1], default cos(match_threshold_angle): least cosine between the two gradients */
  double norm_tol;   /* >= 0, default match_threshold_norm: largest |gn' / gn - 1| */
  double q_abs;      /* >= 0, default 0: added in quadrature to sigma_rho before the update */
  int reserved;      /* 0 */
} rebvio_hip_stereo_prior_opts;
typedef struct rebvio_hip_stereo_prior_counts {
  int candidates; /* the left map's size */
  int usable;     /* keylines with a usable direction */
  int seen;       /* ...with at least one candidate in the window */
  int fused;      /* ...updated */
  int gated;      /* seen, but no candidate inside the gate, or a non-finite update (left as they were) */
  int ambiguous;  /* the gate's candidates spread over more than ambig_px (left as they were) */
  int clamped;    /* among fused: rho ran into RHO_MIN or RHO_MAX */
  int reserved;   /* 0 */
} rebvio_hip_stereo_prior_counts;
/* ctx NULL: cos_min = cos(45 degrees), norm_tol = 1, the default context's. */
void rebvio_hip_default_stereo_prior_opts(rebvio_hip_ctx* ctx /*NULL ok*/, rebvio_hip_stereo_prior_opts* opts);
int rebvio_hip_map_fuse_stereo(rebvio_hip_map* left, rebvio_hip_map* right, const rebvio_hip_stereo_prior_opts* opts,
                               rebvio_hip_stereo_prior_counts* counts, int* outcome_host /*NULL ok*/, int* winner_host /*NULL ok*/);
int rebvio_hip_map_fuse_stereo_async(rebvio_hip_ctx* ctx, rebvio_hip_map* left, rebvio_hip_map* right,
                                     const rebvio_hip_stereo_prior_opts* opts);
int rebvio_hip_stereo_prior_last_counts(rebvio_hip_ctx* ctx, rebvio_hip_stereo_prior_counts* counts);
int rebvio_hip_test_stereo_prior_host(int rows, int cols, float fm, rebvio_hip_keyline* left /*in/out*/, int n,
                                      const rebvio_hip_keyline* right, int nr, const int* right_mask,
                                      const rebvio_hip_stereo_prior_opts* opts, rebvio_hip_stereo_prior_counts* counts,
                                      int* outcome /*NULL or n ints*/, int* winner /*NULL or n ints*/);

/* Place recognition: a fixed-size signature of a map's edges, and a device-resident database of such signatures that is searched in
 * one pass - the retrieval step in front of rebvio_hip_map_keyframe_align_many, which has to be told which old keyframes to try.
 * (The reference has nothing of the kind: it tracks frame to frame and never looks back.)
 *
 * Signature: REBVIO_HIP_PLACE_WORDS = 384 unsigned 16-bit words, 8 x 6 image cells x 8 orientation bins, from the keylines i < size
 * of a map as the map holds them in stream order - pos, gradient, gradient_norm, the fields rebvio_hip_map_upload replaces and
 * rebvio_hip_map_download returns. A keyline is COUNTED when all of these hold (positive tests: a NaN fails)
 *   pos.x >= 0, pos.x < cols, pos.y >= 0, pos.y < rows;  gradient_norm > 0;  |gx| < inf, |gy| < inf;  |gx| > 0 or |gy| > 0
 * and then, with xi = (int)pos.x, yi = (int)pos.y,
 *   cell = ((yi * 6) / rows) * 8 + (xi * 8) / cols                      (integer division)
 *   bin  = 4 * (gy < 0) + 2 * (gx < 0) + (|gy| > |gx|)                  (-0.0 < 0 is false; a tie |gy| == |gx| gives 0)
 *   h[cell * 8 + bin] += 1
 * With n the number of counted keylines sig[k] = (uint16)(((uint64)h[k] * 65535) / n); every word is 0 when n == 0. counted = n
 * goes out next to the signature. There is no transcendental and no floating-point sum: only integer sums cross threads, so
 * every word is the same on every run and equals a host restatement exactly.
 * The gradients of a map that has served as a pair's OLD map are rotated in place; the signature is of what the map holds at that
 * point. The intended place is where the keyframe mark and the snapshot are taken. A map promised to R_prior_next
 * (rebvio_hip_track_pair_finish_async) is refused with -7, as its cloud and its snapshot are.
 *
 * Distance: d(a, b) = sum over the 384 words of |a[k] - b[k]|, a uint32; any u16 words are legal, so d <= 384 * 65535.
 *
 * Database: a rebvio_hip_place_db belongs to a context and holds `cap` signature rows of 768 bytes in device memory, cap in
 * 1..65536 (one owned allocation, plus one for the distances, the counted words and the results; both count in
 * rebvio_hip_test_live_resources and are freed with the handle or with the context, whichever goes first), and on the host its
 * size and a uint64 tag per entry. The handle may outlive its context as a husk: every entry then answers -10 and
 * rebvio_hip_place_db_release still deletes it.
 *
 * Query: among the eligible entries e < size - exclude_last the k with the smallest (distance, index), ascending, k in
 * 1..REBVIO_HIP_PLACE_TOPK_MAX = 16; a tie goes to the lower index; *count = min(k, eligible). An empty eligible set gives
 * *count = 0 and launches nothing.
 *
 * Launches, whatever the sizes: a signature is one clear, k_place_hist (one thread per keyline, workgroups of 256, the map's size
 * read on the device, a 384-word LDS histogram per workgroup) and k_place_norm (one workgroup; writes the u16 words straight into
 * the context's query row or into row `index` of the database); a query adds k_place_dist (one wave per row, the query row in
 * registers), k_place_topk (one workgroup) and one copy of the count and k records. All on the context's track stream under the
 * thread rule of rebvio_hip_map_keyframe_snapshot and rebvio_hip_map_keyframe_align. The first signature gives the context one more
 * owned device allocation (the histogram, the query row and its counted word; kept until the context goes).
 *   rebvio_hip_map_place_signature         synchronous.
 *   rebvio_hip_place_db_create / _release  release once; safe after rebvio_hip_destroy.
 *   rebvio_hip_place_db_clear / _size      size 0 again (the rows stay allocated) / the entries held (-3 as a negative: null handle).
 *   rebvio_hip_place_db_add                queued, no host wait: the signature of `map` becomes row *index = the old size, with `tag`.
 *                                          -7 when the database is full.
 *   rebvio_hip_place_db_add_signature      synchronous upload of a row and its counted word: restores a saved database.
 *   rebvio_hip_place_db_entry              synchronous: row `index`, its counted word and its tag (each output NULL ok). After a
 *                                          queued _add this is the first place that learns that entry's counted; it waits for the stream.
 *   rebvio_hip_place_db_query              the signature of `map` (as rebvio_hip_map_place_signature forms it) against the database.
 *   rebvio_hip_place_db_query_signature    the same from 384 words of the caller's.
 *   rebvio_hip_test_place_signature_host   test hook, touches no device: the signature of n keylines of a rows x cols image.
 *   rebvio_hip_test_place_query_host       test hook, touches no device: the query over `size` rows of 384 words; tag 0 in every record.
 * -3, checked before the device is touched: null arguments; a map of another context than the database's; k outside 1..16, cap
 * outside 1..65536, index outside [0, size); a negative exclude_last or counted; the hooks: a negative size, rows or cols < 1.
 * -10: the context is gone. */
#define REBVIO_HIP_PLACE_WORDS 384
#define REBVIO_HIP_PLACE_TOPK_MAX 16
typedef struct rebvio_hip_place_match {
  uint32_t distance;
  int32_t index; /* the entry's row in the database */
  uint64_t tag;  /* as given when the entry was added */
} rebvio_hip_place_match;
typedef struct rebvio_hip_place_db rebvio_hip_place_db;
int rebvio_hip_map_place_signature(rebvio_hip_map* map, uint16_t* sig /*384*/, int* counted);
int rebvio_hip_place_db_create(rebvio_hip_ctx* ctx, int cap, rebvio_hip_place_db** out);
void rebvio_hip_place_db_release(rebvio_hip_place_db* db);
int rebvio_hip_place_db_clear(rebvio_hip_place_db* db);
int rebvio_hip_place_db_size(rebvio_hip_place_db* db);
int rebvio_hip_place_db_add(rebvio_hip_place_db* db, rebvio_hip_map* map, uint64_t tag, int* index /*NULL ok*/);
int rebvio_hip_place_db_add_signature(rebvio_hip_place_db* db, const uint16_t* sig /*384*/, int counted, uint64_t tag, int* index /*NULL ok*/);
int rebvio_hip_place_db_entry(rebvio_hip_place_db* db, int index, uint16_t* sig /*384, NULL ok*/, int* counted /*NULL ok*/,
                              uint64_t* tag /*NULL ok*/);
int rebvio_hip_place_db_query(rebvio_hip_place_db* db, rebvio_hip_map* map, int k, int exclude_last, rebvio_hip_place_match* out /*k*/,
                              int* count);
int rebvio_hip_place_db_query_signature(rebvio_hip_place_db* db, const uint16_t* sig /*384*/, int k, int exclude_last,
                                        rebvio_hip_place_match* out /*k*/, int* count);
int rebvio_hip_test_place_signature_host(int rows, int cols, const rebvio_hip_keyline* keylines, int n, uint16_t* sig /*384*/, int* counted);
int rebvio_hip_test_place_query_host(const uint16_t* rows384, int size, const uint16_t* sig /*384*/, int k, int exclude_last,
                                     rebvio_hip_place_match* out /*k*/, int* count);

/* Depth hand-over between keyframe snapshots: what the fusion above has made of a retiring keyframe's rho / sigma_rho is lost when
 * the next keyframe is marked - the successor's snapshot is cut from the tracker's map and starts with the tracker's raw depths.
 * rebvio_hip_kf_snapshot_handover_depth carries the refined depths over, as forwardMatch + updateInverseDepth carry depth from map
 * to map per pair (rebvio/src/edge_map.cpp, core.cpp): `src`, the outgoing snapshot, is looked up in the distance field of `map`,
 * the map the new keyframe was marked on; through those associations its depths are propagated into the map's camera frame and
 * written into `dst`, the successor's snapshot, where they are better than what it has. dst must have been taken from `map` (the
 * caller's contract, as for the normals: keyline i of the map is slot i of dst). src is never written. (R, t) is the pose
 * X_cur = R X_kf + t of src against map, e.g. the one rebvio_hip_map_keyframe_align returned. Its uncertainty is NOT propagated:
 * sig_c below is the keyline's own sigma seen from the new frame, nothing more.
 * The two estimates of a slot are NEVER combined: both descend from the tracker's filter (the keyframe's through its mark, the
 * map's through the forward matches), and a Kalman merge would count that ancestry twice - the reason the fusion above refuses the
 * map's rho as a measurement. The better one stands, whole.
 * fp64 behind the loads, every + - * / and sqrt one IEEE operation in the order written. RHO_MIN / RHO_MAX are the fusion's.
 * Pass 1, per src keyline j < src size:
 *   1. steps 1..6 of rebvio_hip_map_keyframe_align at (R, t), with kf_filter, min_cos and max_dist of these options, give the owner
 *      i - or the keyline is not associated. It is not associated either when !(i < dst size) (read on the device).
 *   2. with Z, Y, rho of the term of rebvio_hip_map_keyframe_pose:
 *        rho_c = rho / Y.z                                   (the keyline's inverse depth in the map's frame)
 *        d     = Z.z / (Y.z * Y.z)                           (d rho_c / d rho, since Y.z = Z.z + rho t.z)
 *        s     = (double)sigma_rho_j;   sig_c = fabs(d) * sqrt(s * s + q_abs * q_abs)
 *      out of range unless rho_c and sig_c are finite, sig_c >= 0 and RHO_MIN <= rho_c <= RHO_MAX (positive tests: a NaN drops it).
 *   3. (float)rho_c, (float)sig_c and matches_j are staged, and the keyline claims slot i with a 64-bit integer minimum of
 *      (bits of (float)sig_c) << 32 | j: the smallest propagated sigma wins, the smallest j among equals.
 * Pass 2, per dst keyline i < dst size whose slot was claimed, rc and sc the winner's staged floats, rho_i / sigma_i the slot's:
 *   4. dr = (double)rc - (double)rho_i;   conflict unless dr * dr <= (gate_sigma * gate_sigma) * ((double)sc * sc + (double)sigma_i *
 *      sigma_i) (a positive test: a NaN in dst is a conflict). Two estimates of one edge that disagree beyond their sigmas are two edges.
 *   5. adopted when sc < sigma_i (fp32, strictly): dst gets rho = rc, sigma_rho = sc, matches = max(matches_i, matches_j).
 *      Otherwise kept.
 *   6. pos_img and the normals of dst are never written; a slot that is not adopted keeps all its bits.
 * assoc[j] = i for the winner of an adopted slot; -1 - i for a loser, for out of range and for the winner of a kept or conflicting
 * slot; INT_MIN when not associated. claimed counts slots: claimed = adopted + kept + conflicts, and associated - out_of_range -
 * claimed is the number of losers. Only integer atomics, no floating-point value crosses threads: every output word is the same
 * on every run.
 * Two kernels on the track stream (k_kf_handover_claim: one thread per src keyline; k_kf_handover_apply: one per dst keyline;
 * workgroups of 256, at most 256 of them with a stride loop behind, sizes read on the device). In front of them one all-ones fill of
 * the claim words and one clear of the count block, behind them one copy back (two with assoc_host). Queued while both snapshots'
 * locks are held. Synchronous and track-side; map acceptance as rebvio_hip_kf_snapshot_fuse_depth (-7 where the field is not
 * detection's). The first call that reaches the device gives the context ONE more device allocation (keylines_max claim words,
 * staging records and association words, and the counts: one more live resource, kept until the context goes); none per call. A src
 * of size 0: all counts zero, nothing launched or allocated.
 * -3, before the device is touched: null dst, src, map, R, t or out; dst == src; snapshots or a map of different contexts; a
 * non-finite R or t; an invalid kf_filter; gate_sigma not > 0; q_abs < 0 or NaN; min_cos outside [-1, 1]; max_dist outside
 * 0..search_range; reserved != 0. -10: the context has been destroyed. opts NULL = the defaults.
 * rebvio_hip_test_kf_handover_host (test hook, touches no device): the same statements on the host, in index order, over the arrays of
 * rebvio_hip_test_kf_fuse_host for src (read only) and dst_prs4 / dst_matches (dst_size records, updated in place); opts NULL = the
 * defaults with max_dist = search_range. */
typedef struct rebvio_hip_kf_handover_opts { /* defaults from rebvio_hip_default_kf_handover_opts */
  rebvio_hip_cloud_filter kf_filter;         /* src side, as in rebvio_hip_kf_align_opts; default = default cloud filter */
  double min_cos;                            /* as in rebvio_hip_kf_align_opts, default 0.9 */
  double gate_sigma;                         /* > 0; default 3.0: the conflict gate in standard deviations */
  double q_abs;                              /* >= 0; default 0: added in quadrature to sigma_rho before it is propagated */
  int max_dist;                              /* 0..search_range, default search_range */
  int reserved;                              /* 0 */
} rebvio_hip_kf_handover_opts;
typedef struct rebvio_hip_kf_handover {
  int candidates;     /* src's size */
  int associated;     /* src keylines with an owner below dst's size */
  int out_of_range;   /* ...whose propagated depth is not a usable one (they claim nothing) */
  int claimed;        /* dst slots with at least one claimant */
  int adopted;        /* ...that took the winner's depth */
  int kept;           /* ...that agreed with it and were no worse */
  int conflicts;      /* ...that disagreed with it beyond the gate */
} rebvio_hip_kf_handover;
void rebvio_hip_default_kf_handover_opts(rebvio_hip_ctx* ctx /*NULL: max_dist = 40, the default*/, rebvio_hip_kf_handover_opts* opts);
int rebvio_hip_kf_snapshot_handover_depth(rebvio_hip_kf_snapshot* dst, rebvio_hip_kf_snapshot* src, rebvio_hip_map* map,
                                          const rebvio_hip_kf_handover_opts* opts, const double R[9], const double t[3],
                                          rebvio_hip_kf_handover* out, int* assoc_host /*NULL or src-size ints*/);
int rebvio_hip_test_kf_handover_host(float fm, float cx, float cy, int rows, int cols, int search_range, const float* src_prs4,
                                     const unsigned* src_matches, const float* src_normals /*NULL: none*/, int kf_size,
                                     const float* cur_pos, const float* cur_unit, int n_cur, const int* df_id, const int* df_dist,
                                     float* dst_prs4 /*in/out*/, unsigned* dst_matches /*in/out*/, int dst_size,
                                     const rebvio_hip_kf_handover_opts* opts, const double R[9], const double t[3],
                                     rebvio_hip_kf_handover* out, int* assoc /*NULL or kf_size ints*/);

/* Point cloud of a keyframe snapshot: its depth-bearing keylines - as marked, or as rebvio_hip_kf_snapshot_fuse_depth has refined
 * them - filtered and posed on the device by kernels of their own (the compaction of rebvio_hip_map_point_cloud over the snapshot's
 * buffers; nothing of the map's kernels changes). Per snapshot keyline j < size, with pos_img_j, rho_j, sigma_rho_j, matches_j as the
 * snapshot holds them when the extraction runs in track-stream order (every fusion queued before it is seen, none queued after it):
 *   filter    the test of rebvio_hip_map_point_cloud, term for term: matches >= min_matches, rho >= rho_min, rho <= rho_max,
 *             sigma_rho <= max_rel_sigma * rho (one rounded fp32 multiply); a NaN fails; invalid filters are refused by its rules
 *   position  its formula, operation for operation, fp32, no contraction, fm of the context's parameters:
 *               u = pos_img[0] / fm;  v = pos_img[1] / fm;  z = scale / rho;  xc = u * z;  yc = v * z;
 *               xyz[i] = ((R[3i] * xc + R[3i+1] * yc) + R[3i+2] * z) + t[i]
 *             pose NULL = identity, zero, 1: the cloud in the keyframe's own frame in keyframe depth units, the units of
 *             rebvio_hip_kf_pose::t
 *   record    rebvio_hip_cloud_point: rho, sigma_rho, matches as stored in the snapshot; keyline = j, strictly increasing, and the
 *             index into rebvio_hip_kf_snapshot_download / _download_normals (a consumer joins the normals through it);
 *             gradient_norm = +0.0f: a snapshot does not keep the gradient norm
 * *count = keylines that pass; min(count, cap) records are written (a cap below count is no error). No atomic decides a place:
 * the cloud is reproducible bit for bit.
 * Both entries are track-side and follow the calling rules of rebvio_hip_map_keyframe_snapshot; the queued one is allowed between
 * _finish_async(k) and _begin(k+1) and waits for nothing on the host (the size is read on the device: a snapshot of size 0 gives
 * count 0). It returns a handle of the kind rebvio_hip_map_point_cloud_async returns: rebvio_hip_cloud_wait / _release serve it
 * unchanged (device_points, -12, -10), and buffers, stream and stamps are the context's cloud pool, whichever kind of cloud made
 * them. A snapshot has no R_prior_next state: there is no -7. The snapshot may be released right after the queued call.
 * -3, before the device is touched: null snapshot / count / out, negative cap, null points with cap > 0, an invalid filter, NaN in
 * the pose; -10: the context has been destroyed.
 * rebvio_hip_test_kf_cloud_host (test hook, touches no device): the same per-record statement on the host over caller arrays
 * (snap_prs4 = kf_size records of pos_img.x, pos_img.y, rho, sigma_rho) in index order; -3 for null arrays (kf_size > 0), a negative
 * size and whatever the device entry refuses. */
int rebvio_hip_kf_snapshot_point_cloud(rebvio_hip_kf_snapshot* snap, const rebvio_hip_cloud_filter* filter,
                                       const rebvio_hip_cloud_pose* pose, rebvio_hip_cloud_point* points_host, int cap, int* count);
int rebvio_hip_kf_snapshot_point_cloud_async(rebvio_hip_kf_snapshot* snap, const rebvio_hip_cloud_filter* filter,
                                             const rebvio_hip_cloud_pose* pose, rebvio_hip_cloud** out);
int rebvio_hip_test_kf_cloud_host(float fm, const float* snap_prs4, const unsigned* snap_matches, int kf_size,
                                  const rebvio_hip_cloud_filter* filter, const rebvio_hip_cloud_pose* pose,
                                  rebvio_hip_cloud_point* points, int cap, int* count);

/* Test hook: overwrite the device keylines (count must equal the map size). */
int rebvio_hip_map_upload(rebvio_hip_map* m, const rebvio_hip_keyline* keylines, int n);
/* Test hook: overwrite the device's dense mask (rows * cols ints, each -1 or a keyline index below the map's size; -3 otherwise) - with
 * rebvio_hip_map_upload a right map for rebvio_hip_map_fuse_stereo planted by hand. The map's distance field is not rebuilt: such a
 * map is not for tracking. */
int rebvio_hip_test_map_set_mask(rebvio_hip_map* m, const int* mask);
/* Map handles may outlive their context: after rebvio_hip_destroy the entries that take a map alone (size, threshold, download,
 * render, upload, map_distance_field) fail with -10 (NaN for the threshold) and rebvio_hip_map_release frees what is left of the
 * handle - nothing of the destroyed context is touched. (A handle must still be released exactly once.) */
void rebvio_hip_map_release(rebvio_hip_map* m);

/* Core::buildDistanceField / DistanceField::build (core.cpp:33-37, core.hpp:37-59). */
int rebvio_hip_build_distance_field(rebvio_hip_ctx* ctx, rebvio_hip_map* m);
/* DistanceField::operator[] for all cells (core.hpp:61): ids (-1 = none) and distances (valid where id >= 0). */
int rebvio_hip_distance_field(rebvio_hip_ctx* ctx, int* id_out, int* dist_out);

/* rebvio::DistanceField::operator[] (core.hpp:61) for the field built FROM map `m` (by detect, or by
 * rebvio_hip_build_distance_field): the field lives with its map, so it stays readable while the map is alive. */
int rebvio_hip_map_distance_field(rebvio_hip_map* m, int* id_out, int* dist_out);

/* EdgeMap::searchMatch (edge_map.hpp:93-94, edge_map.cpp:101-184): searched->searchMatch(query, vel, Rvel, Rback, max_radius),
 * one keyline of another map against `searched`. vel / Rvel are used as given (directedMatch passes them rotated by Rback,
 * edge_map.cpp:193-194). *idx_out = index of the match in `searched`, or -1. Synchronises. */
int rebvio_hip_search_match(rebvio_hip_ctx* ctx, rebvio_hip_map* searched, const rebvio_hip_keyline* query, const float vel[3],
                            const float Rvel[9], const float Rback[9], float max_radius, int* idx_out);

/* FastGaussian::smooth (scale_space.hpp:31, scale_space.cpp:173-182) on a host fp32 image: three integral-image box
 * passes of the given (odd, 3..11) widths, as FastGaussian's constructor derives them from sigma (scale_space.cpp:14-41).
 * Test/diagnostic entry like rebvio_hip_scale_space. */
int rebvio_hip_smooth(rebvio_hip_ctx* ctx, const float* img_host, const int widths3[3], float* out_host);
/* The same for FastGaussian's general n (scale_space.cpp:14-41 takes any number of box passes; the reference itself only uses
 * n = 3, scale_space.cpp:186): n in 1..16 passes of the given odd widths in 3..11. */
int rebvio_hip_smooth_n(rebvio_hip_ctx* ctx, const float* img_host, const int* widths, int n, float* out_host);

/* EdgeMap::rotateKeylines (edge_map.cpp:58-71); R row-major 3x3. */
int rebvio_hip_rotate(rebvio_hip_ctx* ctx, rebvio_hip_map* m, const float R[9]);
/* EdgeMap::estimateQuantile (edge_map.cpp:39-56). */
int rebvio_hip_quantile(rebvio_hip_ctx* ctx, rebvio_hip_map* m, float percentile, int num_bins, float* out);
/* Core::tryVel (core.cpp:78-148). `residuals` (host, map-size floats) is read and updated like the
 * reference's `_residuals`; out10 = score, JtJ(0,0),(1,1),(2,2),(0,1),(0,2),(1,2), JtF[0..2]. */
int rebvio_hip_try_vel(rebvio_hip_ctx* ctx, rebvio_hip_map* m, const float vel[3], float sigma_rho_min,
                       float* residuals, float out10[10]);
/* Core::minimizeVel (core.cpp:150-189) with the Levenberg-Marquardt loop kept on the device.
 * vel is in/out; Rvel = invert(JtJ); returns score in *F. */
int rebvio_hip_minimize_vel(rebvio_hip_ctx* ctx, rebvio_hip_map* m, float vel[3], float Rvel[9], float* F,
                            int* accept_mask, float* sigma_rho_min);
/* EdgeMap::forwardMatch (edge_map.cpp:73-99): old_map->forwardMatch(new_map). Depends on nothing but old_map's match_id_forward
 * and the two maps' keylines as they stand at the call, like the reference's: it may be repeated, follow any number of
 * rebvio_hip_minimize_vel / rebvio_hip_try_vel calls or an upload of either map, and go into a new_map that already holds matches -
 * a target that is matched and holds a larger rho than its best writer keeps its fields (edge_map.cpp:83). (Per target the
 * writer of largest rho wins, the largest index among equals: what the reference's walk in index order comes to.) */
int rebvio_hip_forward_match(rebvio_hip_ctx* ctx, rebvio_hip_map* old_map, rebvio_hip_map* new_map);
/* Core::extRotVel (core.cpp:191-261) on the distance field's map. JtJ 6x6 row-major, JtF[6], X[6]. */
int rebvio_hip_ext_rot_vel(rebvio_hip_ctx* ctx, const float vel[3], float Wx[36], float JtF[6], float X[6], int* ok);
/* EdgeMap::directedMatch (edge_map.cpp:186-218): new_map->directedMatch(old_map, ...). -3 when max_radius is outside 0..255 or
 * max_radius + 2 * pixel_uncertainty_match + 2 exceeds 260 (the bound rebvio_hip_create puts on search_range). */
int rebvio_hip_directed_match(rebvio_hip_ctx* ctx, rebvio_hip_map* new_map, rebvio_hip_map* old_map, const float vel[3],
                              const float Rvel[9], const float Rback[9], float max_radius, int* matches,
                              int* kf_matches);
/* EdgeMap::regularize1Iter (edge_map.cpp:220-259). */
int rebvio_hip_regularize(rebvio_hip_ctx* ctx, rebvio_hip_map* m, int* count);
/* Core::updateInverseDepth (core.cpp:417-456) on the distance field's map. */
int rebvio_hip_update_inverse_depth(rebvio_hip_ctx* ctx, const float vel[3]);

/* Gyro-bias state of the frame-pair glue (types/imu.hpp:180-183) back to its initial value. */
void rebvio_hip_reset_state(rebvio_hip_ctx* ctx);
/* imu_state_.Bg / imu_state_.W_Bg (types/imu.hpp:180-182): read / set by the orchestrator's gyro-bias initialisation
 * (rebvio.cpp:146-160). */
int rebvio_hip_get_gyro_state(rebvio_hip_ctx* ctx, float Bg[3], float W_Bg[9]);
int rebvio_hip_set_gyro_state(rebvio_hip_ctx* ctx, const float Bg[3], const float W_Bg[9]);
/* One frame pair, rebvio.cpp:142-259 (accelerometer/SAB branch excluded): distance field of new_map
 * (if not yet built), rotate, minimizeVel, forwardMatch, extRotVel, gyroBiasCorrection, rotate,
 * directedMatch, regularize1Iter, updateInverseDepth. R_prior = IMU inter-frame rotation or NULL.
 * forwardMatch inside a pair (here, in rebvio_hip_track_pair_begin and in the streaming / batch pushes): the winners are
 * published by the pair's last tryVel evaluation into new_map, and edge_map.cpp:83 holds as in rebvio_hip_forward_match - a
 * new_map keyline that comes in matched keeps its fields against a writer of smaller rho. What a pair does NOT do is forget the
 * winners of an earlier pair: new_map must not have been the new map of an earlier pair (or of a rebvio_hip_minimize_vel whose
 * distance field it was) since it was detected. The drivers always hand over a map fresh from detection; tracking one new map
 * a second time through the pair entries is not supported - use the stepwise calls, whose rebvio_hip_forward_match starts from
 * match_id_forward alone. */
int rebvio_hip_track_pair(rebvio_hip_ctx* ctx, rebvio_hip_map* old_map, rebvio_hip_map* new_map, const float* R_prior,
                          float frame_dt, rebvio_hip_pair_out* out);

/* The same step in two halves, for hosts that fuse inertial data between them (rebvio.cpp:206-233: accelerometer /
 * scale-attitude-bias filter decides the final V, Rgva and the second rotation):
 *   begin  = rebvio.cpp:142-191: distance field, rotate by the gyro prior, minimizeVel, forwardMatch, extRotVel,
 *            gyroBiasCorrection. Returns Vg, P_Vg, Xv, W_Xv, Xgv, W_Xgv (after correction) and R (prior corrected by Bg).
 *            (new_map: not the new map of an earlier pair, see rebvio_hip_track_pair.)
 *   finish = rebvio.cpp:223/232 + 236-259: rotate the old map by R_second, directedMatch with (V, P_V, Rgva),
 *            regularize1Iter, updateInverseDepth; status 0 / 1 (NaN in V) / 2 (< global_min_matches_threshold). */
typedef struct rebvio_hip_pair_mid {
  float Vg[3];
  float P_Vg[9];
  float F;
  float sigma_rho_min;
  int lm_accept_mask;
  int ext_ok;
  float Xv[6];
  float W_Xv[36];
  float Xgv[6];
  float W_Xgv[36];
  float R[9];
} rebvio_hip_pair_mid;
int rebvio_hip_track_pair_begin(rebvio_hip_ctx* ctx, rebvio_hip_map* old_map, rebvio_hip_map* new_map, const float* R_prior,
                                float frame_dt, rebvio_hip_pair_mid* mid);
int rebvio_hip_track_pair_finish(rebvio_hip_ctx* ctx, rebvio_hip_map* old_map, rebvio_hip_map* new_map, const float V[3],
                                 const float P_V[9], const float Rgva[9], const float R_second[9], int* klm_num,
                                 int* kf_matches, int* reg_num, int* status);
/* _finish in two steps, so that a host can queue the NEXT pair's first half behind this pair's second half before it waits for
 * anything: _finish_async hands over the fusion's results and returns at once; _result waits for the second half and returns
 * its counters / status (what rebvio.cpp:245-259 needs for the "insufficient matches" stop and what the odometry record carries).
 * Allowed order: begin(k), finish_async(k), begin(k+1), result(k), finish_async(k+1), ... - one result may be outstanding.
 * Between _begin and _finish(_async) of a pair only _result of the previous pair may be called. Between _finish_async(k) and
 * _begin(k+1) rebvio_hip_map_point_cloud_async is allowed as well (it queues behind pair k and waits for nothing).
 * A pair's match counters ride to the host in the NEXT pair's first-half record when that pair continues from this pair's new
 * map (no copy, no extra wait); otherwise _begin / _result copy them. (Releasing that map before _result is allowed: the
 * release copies them out first.) */
/* R_prior_next (may be NULL): the IMU inter-frame rotation the NEXT pair's _begin will be given as R_prior, when the caller
 * already has it. That pair's first rotateKeylines (rebvio.cpp:163-165) then runs inside this pair's last kernel and its
 * _begin launches one kernel less. R_prior_next is a promise: the old map is rotated in place with it, so the next _begin must
 * be given the same R_prior and must find the gyro state this pair's _begin left (no rebvio_hip_set_gyro_state / _reset_state
 * in between); otherwise it returns -7 and that pair cannot be tracked from this map any more. */
int rebvio_hip_track_pair_finish_async(rebvio_hip_ctx* ctx, rebvio_hip_map* old_map, rebvio_hip_map* new_map, const float V[3],
                                       const float P_V[9], const float Rgva[9], const float R_second[9], const float* R_prior_next);
int rebvio_hip_track_pair_result(rebvio_hip_ctx* ctx, int* klm_num, int* kf_matches, int* reg_num, int* status);
/* Optional, before _finish(_async) of a pair: the map the NEXT pair will track as its new map (already handed to detect).
 * The track stream's wait for that map's detection is queued now, ahead of this pair's second half, instead of between the two
 * pairs (one barrier packet less on the pair-to-pair path). The reference has no counterpart: its maps are host objects. */
int rebvio_hip_track_pair_hint_next(rebvio_hip_ctx* ctx, rebvio_hip_map* next_new_map);

/* Streaming driver used by the bench: a software pipeline, detect(frame) on the scan / keyline streams overlapped with
 * the tracking of EARLIER pairs on the track stream. A pair runs on the device from end to end: the glue between its halves
 * (6x6 solve, gyroBiasCorrection, SO3, covariance: rebvio.cpp:177-233 without the accelerometer branch) is evaluated in front
 * of the directedMatch kernel from the first half's records, with the gyro-bias state kept in device memory, so the host only
 * queues launches and reads records. (Every pair's new map is fresh from detection here and in the batch pushes, which is what
 * forwardMatch inside a pair expects: see rebvio_hip_track_pair.) `out` receives the oldest COMPLETE pair not handed out yet, in pair order, several calls
 * behind `frame` (the detect stage leads the tracker by REBVIO_HIP_LEAD frames, default 5; pairs are queued on the track stream
 * in groups of REBVIO_HIP_GROUP, default 4, with one stream wait and one event per group; a pair's match counters arrive with
 * the next pair; up to fifteen pairs are in flight between the device and the host); status -1 while there is none.
 * rebvio_hip_flush() tracks the pairs not started yet and finishes everything in flight: a stream of n frames yields n - 1
 * records; those not handed out by a push are fetched with rebvio_hip_next_record: 1 = *out / *keylines filled, 0 = none left.
 * rebvio_hip_get_gyro_state follows the stream with that lag and is exact after a flush; rebvio_hip_set_gyro_state is refused
 * (-7) while frames are in flight. */
int rebvio_hip_push_frame_u8_device(rebvio_hip_ctx* ctx, const uint8_t* frame_dev, uint64_t ts_us,
                                    rebvio_hip_pair_out* out, int* keylines);
/* The same for a MONO8 frame in HOST memory (what imageCallback is handed, rebvio.cpp:38-48): copied into a pinned ring here
 * (the caller's buffer is free when the call returns) and from there to the device ahead of the frame's scans, in stream order. */
int rebvio_hip_push_frame_u8(rebvio_hip_ctx* ctx, const uint8_t* frame_host, size_t pitch_bytes, uint64_t ts_us,
                             rebvio_hip_pair_out* out, int* keylines);
/* The two push entries for a frame of any REBVIO_HIP_PX_* format (see rebvio_hip_detect_px). */
int rebvio_hip_push_frame_px(rebvio_hip_ctx* ctx, const void* frame_host, size_t pitch_bytes, int fmt, uint64_t ts_us,
                             rebvio_hip_pair_out* out, int* keylines);
int rebvio_hip_push_frame_px_device(rebvio_hip_ctx* ctx, const void* frame_dev, int fmt, uint64_t ts_us,
                                    rebvio_hip_pair_out* out, int* keylines);
/* push_frame_px_device with a per-frame detection mask (rows*cols bytes in device memory; see rebvio_hip_set_detection_mask). */
int rebvio_hip_push_frame_px_masked_device(rebvio_hip_ctx* ctx, const void* frame_dev, int fmt, const uint8_t* mask_dev, uint64_t ts_us,
                                           rebvio_hip_pair_out* out, int* keylines);
/* The push entries for a camera with an IMU: the reference starts every pair from the gyro - imu.R(), corrected by the bias
 * estimate, rotates the old keylines ahead of minimizeVel (rebvio.cpp:163-165), and gyroBiasCorrection weighs the visual rotation
 * against that measurement (rebvio.cpp:186-190). R_gyro: 9 floats, row-major, the gyro rotation pre-integrated over the interval
 * from the frame pushed before this one to this frame - exactly R_prior of rebvio_hip_track_pair for the pair that ENDS at this
 * frame (rebvio_hip_gyro_integrate forms it from rate samples). The records equal those of rebvio_hip_track_pair(map_k, map_k+1,
 * R_gyro(k+1), ...) on the same frames bit for bit, and rebvio_hip_get_gyro_state after a flush likewise. NULL = identity = what
 * the entries above push; a stream's first frame has no earlier frame and its rotation is ignored. mask_dev: per-frame detection
 * mask as rebvio_hip_push_frame_px_masked_device takes it, or NULL for none. Frame, format, pitch and mask are checked as by the
 * *_px entries; a non-finite entry of R_gyro is refused (-3, rebvio_hip_last_error names the argument) before anything is
 * queued. There is no orthonormality check, as R_prior has none.
 * Flushes: a pair's last kernel applies the NEXT pair's first rotation, which needs the rotation of the frame behind it. The last
 * pair in front of a rebvio_hip_flush cannot know it. From the first non-NULL R_gyro on a context is a gyro stream and stays one:
 * its flush leaves the newest map un-rotated and KEEPS it, and the next frame pushed continues the stream from it (its R_gyro spans
 * the interval from that map's frame; n frames around any number of flushes yield n - 1 records; rebvio_hip_reset_state ends the
 * stream). A context that has never been given a rotation flushes as before: the stream ends, its newest map rotated for an
 * identity measurement. A rotation that is not bit for bit the identity, pushed right after such a flush, has no frame to be
 * measured from and is refused (-7); NULL or the identity start the new stream. */
int rebvio_hip_push_frame_px_gyro_device(rebvio_hip_ctx* ctx, const void* frame_dev, int fmt, const uint8_t* mask_dev /*NULL = none*/,
                                         const float* R_gyro /*NULL = identity*/, uint64_t ts_us, rebvio_hip_pair_out* out, int* keylines);
int rebvio_hip_push_frame_px_gyro(rebvio_hip_ctx* ctx, const void* frame_host, size_t pitch_bytes, int fmt, const float* R_gyro,
                                  uint64_t ts_us, rebvio_hip_pair_out* out, int* keylines);
/* R <- R * exp(gyro_cam * dt_s): one step of IntegratedImu::add (types/imu.hpp:72) with the library's own SO3 exponential, so that a
 * caller holding raw rate samples (rad/s, already rotated into the camera frame: the reference applies R_c2i there) can form
 * R_gyro: start from the identity at a frame and call it once per sample up to the next frame. Host only, touches no device. */
void rebvio_hip_gyro_integrate(float R[9], const float gyro_cam[3], float dt_s);
/* Keyframes in the streaming driver: the next frame pushed, through any push entry, becomes a keyframe (see
 * rebvio_hip_map_mark_keyframe): its map is marked behind the pair that ends at it and in front of the pair that starts from it (a
 * stream's first frame: in front of its first pair; the map a gyro stream carries across a flush keeps the request). On the same
 * frames the records equal those of the per-pair run track_pair(j-1, j); map_mark_keyframe(j); track_pair(j, j+1) in every word. A
 * frame that is dropped untracked (the newest frame of a stream without rotations at its flush) takes its request with it;
 * rebvio_hip_reset_state drops a pending one. A stream that never calls this launches exactly what it launched before. -3: a null
 * context, or a lane of a batch (keyframes inside lock-step steps are not supported). */
int rebvio_hip_keyframe_next(rebvio_hip_ctx* ctx);
int rebvio_hip_next_record(rebvio_hip_ctx* ctx, rebvio_hip_pair_out* out, int* keylines);
/* Frame pairs the streaming driver has queued on the device so far (a measurement aid: pairs are queued in groups, so a short
 * window of pushes may start a few pairs more or fewer than it pushes frames). */
uint64_t rebvio_hip_pairs_started(rebvio_hip_ctx* ctx);
int rebvio_hip_flush(rebvio_hip_ctx* ctx);

/* Several camera streams on ONE GPU, advanced in lock-step ("lanes" of a batch). The reference runs one rebvio::Rebvio per
 * camera stream, each with its own detector, tracker and queues (rebvio.hpp:91-112); a batch is `lanes` such pipelines whose
 * per-frame kernels are launched once per step for all lanes (lane = blockIdx.z). One 640x480 stream keeps well under a tenth
 * of an MI355X busy - its kernels are short latency chains - so a batched step costs about what a single stream's step costs
 * and the frame rate scales with the lane count until the chip fills. Every lane is a full context (own maps, servo, gyro-bias
 * state) sharing the batch's three streams; its records are bit-identical to those of a stand-alone context fed the same
 * frames. lanes in 1..16, any keylines_max a context accepts. The persistent tracking kernel's workgroups exchange records
 * within a lane and must be resident together for that: the driver launches it for as many lanes at a time as the device holds
 * (8 lanes of 16k keylines on an MI355X; 16 lanes take two such launches per step), and rebvio_hip_batch_create refuses (-3)
 * a keylines_max whose single lane does not fit. A lens model (rebvio_hip_set_undistort on every lane's context, or on none) puts the batched front end
 * (x3 + undistort, rebvio.cpp:43-47) ahead of the scans, each lane through its own model.
 * push: frames_dev[l] = this step's u8 frame of lane l in device memory (all lanes share ts_us); out[l] / keylines[l] receive
 * lane l's oldest COMPLETE pair not handed out yet, like rebvio_hip_push_frame_u8_device (status -1 while there is none);
 * after rebvio_hip_batch_flush the remaining steps' records are fetched with rebvio_hip_batch_next_records (1 = filled, 0 = none).
 * A push that fails after some lanes have been prepared leaves the batch out of lock-step: it is marked and every later call
 * returns -11. */
typedef struct rebvio_hip_batch rebvio_hip_batch;
int rebvio_hip_batch_create(const rebvio_hip_params* p, int lanes, rebvio_hip_batch** out);
void rebvio_hip_batch_destroy(rebvio_hip_batch* b);
int rebvio_hip_batch_lanes(rebvio_hip_batch* b);
/* The context of one lane (device_alloc / device_upload for its frames, detector_state, get/set_gyro_state, ...). Owned by the batch. */
rebvio_hip_ctx* rebvio_hip_batch_lane(rebvio_hip_batch* b, int lane);
int rebvio_hip_batch_push_u8_device(rebvio_hip_batch* b, const uint8_t* const* frames_dev, uint64_t ts_us, rebvio_hip_pair_out* out,
                                    int* keylines);
/* The same with every lane's frame in the REBVIO_HIP_PX_* format `fmt` (dense in device memory; see rebvio_hip_detect_px). */
int rebvio_hip_batch_push_px_device(rebvio_hip_batch* b, const void* const* frames_dev, int fmt, uint64_t ts_us,
                                    rebvio_hip_pair_out* out, int* keylines);
/* The same with a per-frame detection mask for every lane: masks_dev[l] = lane l's mask (rows*cols bytes in device memory), or
 * NULL for none (see rebvio_hip_set_detection_mask; a lane's static mask applies as well). */
int rebvio_hip_batch_push_px_masked_device(rebvio_hip_batch* b, const void* const* frames_dev, int fmt, const uint8_t* const* masks_dev,
                                           uint64_t ts_us, rebvio_hip_pair_out* out, int* keylines);
/* The same with a gyro rotation per lane (rebvio_hip_push_frame_px_gyro_device; rebvio.cpp:163-165 per lane): R_gyro = NULL, or
 * one pointer per lane with NULL entries for the identity; masks_dev = NULL, or as above. Between two flushes every lane equals a
 * stand-alone context pushed the same frames and rotations; a lane that is never given one equals a lane of the entries above.
 * Across a flush the two differ: unlike a context's flush, rebvio_hip_batch_flush ends every lane's stream, rotations or not (the
 * lanes stay in lock-step). The step pushed next is every lane's first frame, its rotations are ignored, and the pair across
 * the flush, which a stand-alone context with rotations tracks, does not exist for a lane. */
int rebvio_hip_batch_push_px_gyro_device(rebvio_hip_batch* b, const void* const* frames_dev, int fmt, const uint8_t* const* masks_dev /*NULL or NULL entries*/,
                                         const float* const* R_gyro /*NULL, or one pointer per lane, NULL entries = identity*/,
                                         uint64_t ts_us, rebvio_hip_pair_out* out, int* keylines);
int rebvio_hip_batch_next_records(rebvio_hip_batch* b, rebvio_hip_pair_out* out, int* keylines);
int rebvio_hip_batch_flush(rebvio_hip_batch* b);

/* Test hook: the glue of one pair (rebvio.cpp:177-233 without the accelerometer branch: sum of the extRotVel block records, 6x6
 * solve, gyroBiasCorrection, SO3 correction, covariance, next prior) evaluated on the device, as the streaming and batch drivers
 * run it, AND on the host, as rebvio_hip_track_pair runs it, from the same inputs: final minimizeVel state (vel, the six
 * unique JtJ entries (0,0) (1,1) (2,2) (0,1) (0,2) (1,2), F, sigma_rho_min, accept mask), ceil(n_new / 256) extRotVel records of
 * 32 floats, frame_dt, filter state and prior rotation. Outputs per side: the pair record, the filter state after the pair
 * (22 floats: Bg, W_Bg, next prior rotation, pad) and the second half's inputs (44 words). The two sides must agree bit for bit. */
int rebvio_hip_test_glue(rebvio_hip_ctx* ctx, const float vel[3], const float JtJ6[6], float F, float sigma_rho_min, int accept_mask,
                         const float* xrv, int n_new, float frame_dt, const float Bg[3], const float W_Bg[9], const float R_prior[9],
                         rebvio_hip_pair_out* out_dev, float* state_dev, float* second_dev, rebvio_hip_pair_out* out_host,
                         float* state_host, float* second_host);
/* Test hook: the gyro rotation of the NEXT pair that later rebvio_hip_test_glue calls of this context hand to both forms (what a
 * frame pushed with R_gyro gives the glue of the pair in front of it), and whether it is known (has_next = 0: the last pair in
 * front of a flush on a stream with rotations). R_next = NULL: back to the identity, known. Touches nothing but that hook. */
int rebvio_hip_test_glue_set_next(rebvio_hip_ctx* ctx, const float* R_next, int has_next);

/* Test hook for the sequence stamps of the host-visible pair records. Every pair the library queues carries a non-zero sequence
 * number; the pair's kernels store it as the LAST word of each record they write into host-visible memory (result slot, glue
 * record), and every entry that reads such a record - rebvio_hip_track_pair, _track_pair_begin, _push_frame_u8(_device),
 * _next_record's producer, _flush and the batch forms - compares it first: a record read before its pair wrote it (a completion
 * event or a synchronisation that reported too early) fails with status -12 instead of handing out stale poses. This hook hands
 * the kernels of the NEXT pair (batch: the last lane of the next step) a wrong number, which is exactly what such a record looks
 * like to the reader. */
int rebvio_hip_test_forge_record_stamp(rebvio_hip_ctx* ctx);
int rebvio_hip_batch_test_forge_record_stamp(rebvio_hip_batch* b);

/* Test hook for the streaming driver's hand-over between its streams (REBVIO_HIP_HANDOVER): counts since the context
 * was created. out[3 * s + 0 .. 2], s = 0 track / 1 scan / 2 keyline stream: event waits queued on the stream, waits left out
 * because the host knew their reason gone (keyline stream: the release token of the edge map it reuses had been observed), events
 * recorded on the stream; out[9]: reuses of an edge map whose release token the host had not observed yet (an event is recorded
 * on the track stream then and waited for). */
int rebvio_hip_test_handover_counters(rebvio_hip_ctx* ctx, unsigned long long out[10]);

/* Test hook for leaks: the device buffers, pinned host buffers, events and streams that the contexts, edge maps, point clouds and
 * batches of this process hold right now, as one exact count (not bytes). Creating any of them raises it, destroying a context
 * or a batch lowers it by all that the object took, what it allocated on first use included; a map or cloud handle kept across
 * rebvio_hip_destroy holds none. A process that has destroyed everything it created reads the value it started with. Memory
 * from rebvio_hip_device_alloc belongs to the caller and is not counted, nor are the profiler's pooled events. */
long rebvio_hip_test_live_resources(void);

/* Per-kernel device timing of the last N launches of each kernel, measured with HIP events on the
 * stream the kernel runs on. names: '\n'-separated. Used by bench.py's roofline leg. */
int rebvio_hip_profile_enable(rebvio_hip_ctx* ctx, int on); /* 0 off, 1 every launch, N>1 every N-th launch */
int rebvio_hip_profile_select(rebvio_hip_ctx* ctx, const char* only_kernel); /* NULL/"" = every kernel */
int rebvio_hip_profile_reset(rebvio_hip_ctx* ctx);
int rebvio_hip_profile_read(rebvio_hip_ctx* ctx, char* names, size_t names_cap, double* avg_us, int* calls, int cap);

/* Device memory helpers so that hosts without a HIP runtime binding (ctypes, cgo) can stage frames. */
int rebvio_hip_device_alloc(rebvio_hip_ctx* ctx, size_t bytes, void** out);
int rebvio_hip_device_free(rebvio_hip_ctx* ctx, void* p);
int rebvio_hip_device_upload(rebvio_hip_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif
