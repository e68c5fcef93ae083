/*
 * mage_hot.h — C-ABI of the MI355X-native MAGE-SLAM hot path.
 *
 * This is the drop-in boundary described in SURVEY.md §8(b).  Every entry point takes
 * plain pointers and sizes (no torch, OpenCV, Eigen or g2o types) and replaces one
 * reference interface, cited per function.  Reference paths are relative to the
 * marwie/mageslam tree; `Core/.../Source` = `Core/MAGESLAM/Source`.
 *
 * Status codes replace the reference's CV_Assert / assert failures; the C++ facades
 * (include/mage/mage.hpp) turn them back into exceptions so callers keep the reference
 * behaviour.
 */
#ifndef MAGE_HOT_H
#define MAGE_HOT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mage_status {
    MAGE_OK = 0,
    MAGE_EINVAL = 1,        /* bad argument (reference: CV_Assert / assert) */
    MAGE_EDEVICE = 2,       /* HIP runtime error or no usable gfx950 device */
    MAGE_ENOMEM = 3,        /* device allocation failed */
    MAGE_EUNSUPPORTED = 4,  /* valid reference input this build does not handle yet */
    MAGE_ECAPACITY = 5      /* output capacity too small (outputs are truncated) */
} mage_status;

/* Layout-identical to cv::KeyPoint {Point2f pt; float size, angle, response; int octave, class_id}
 * as stored in ImageData (Core/.../Source/Image/ImageData.h:186-205). 28 bytes. */
typedef struct mage_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} mage_keypoint;

/* Layout-identical to cv::DMatch {int queryIdx, trainIdx, imgIdx; float distance}. 16 bytes. */
typedef struct mage_dmatch {
    int32_t query_idx, train_idx, img_idx;
    float distance;
} mage_dmatch;

/* The 14 constructor scalars of OrbDetector (Core/.../Source/Image/OpenCVModified.h:68-82),
 * same order and meaning; defaults in FeatureExtractorSettings (MageSettings.h:151-167). */
typedef struct mage_orb_settings {
    uint32_t gaussian_kernel_size; /* 7 */
    uint32_t nfeatures;            /* 440 (2000 in the 720p benchmark) */
    float scale_factor;            /* 1.5 */
    uint32_t nlevels;              /* 1 */
    uint32_t patch_size;           /* 15 */
    uint32_t fast_threshold;       /* 4 */
    int32_t use_orientation;       /* 0 */
    float feature_factor;          /* 1.5 (ANMS) */
    float feature_strength;        /* 0.9 (ANMS) */
    int32_t strong_response;       /* 20 (ANMS) */
    float min_robust_factor;       /* 1.1 */
    float max_robust_factor;       /* 2.0 */
    int32_t num_cells_x;           /* 32 */
    int32_t num_cells_y;           /* 32 */
} mage_orb_settings;

/* Pyramid levels supported (nlevels in 1..MAGE_MAX_LEVELS). */
#define MAGE_MAX_LEVELS 8

typedef void* mage_stream; /* a hipStream_t; NULL = the default stream */

/* ------------------------------------------------------------------------------------------ */
/* Library                                                                                      */
/* ------------------------------------------------------------------------------------------ */

/* Version string and the gfx target the device code was compiled for ("gfx950"). */
const char* mage_version(void);
/* Last error message of the calling thread (empty string if none). */
const char* mage_last_error(void);
/* Frees the library's idle cached blocks (device, page-locked and mapped host memory retired by
 * destroyed per-task objects such as mage_ba) on `device` (-1: every device); returns the bytes
 * freed.  The cache keeps at most MAGE_POOL_CAP_MB (default 512) MB of idle device memory, a
 * quarter of that page-locked and a sixteenth mapped, frees blocks no request could use over 256
 * requests, and is trimmed automatically when an allocation fails.  No reference counterpart
 * (the reference allocates per task through new / cv::Mat). */
uint64_t mage_pool_trim(int32_t device);

/* Per-kernel timing: when enabled, every launch is bracketed by HIP events recorded on the
 * stream it is launched on.  The report is one line per kernel: "<name> <launches> <total_ms>". */
void mage_profile_enable(int32_t enable);
/* Time only the launches whose kernel tag starts with tag_prefix (null or "": all of them). */
void mage_profile_filter(const char* tag_prefix);
void mage_profile_reset(void);
const char* mage_profile_report(void);

/* ------------------------------------------------------------------------------------------ */
/* ORB extraction — replaces OrbDetector (Core/.../Source/Image/OpenCVModified.h:64-173)        */
/* ------------------------------------------------------------------------------------------ */

typedef struct mage_orb mage_orb;

/* OrbDetector::OrbDetector (OpenCVModified.cpp:362-393).  Also binds the HIP device. */
mage_status mage_orb_create(const mage_orb_settings* settings, int device, mage_orb** out);
mage_status mage_orb_destroy(mage_orb* orb);

/* OrbDetector::DetectAndCompute (OpenCVModified.cpp:771-886) on one 8-bit gray frame in host
 * memory; synchronous.  Writes up to `cap` keypoints (the ImageData capacity,
 * ImageData.h:65-70 truncates silently) and cap*32 descriptor bytes; *n = count.
 * Keypoint order is the canonical order of DESIGN.md §ORB (ANMS rank, else raster). */
mage_status mage_orb_detect_and_compute(mage_orb* orb, const uint8_t* img, int32_t width,
                                        int32_t height, int32_t stride, mage_keypoint* kp,
                                        uint8_t* desc, uint32_t cap, uint32_t* n);

/* Batched, device-resident form: `batch` frames at d_frames + f*frame_pitch (device memory),
 * outputs at d_kp + f*cap, d_desc + f*cap*32, d_n[f].  Asynchronous on `stream`. */
mage_status mage_orb_detect_and_compute_batch_device(mage_orb* orb, const uint8_t* d_frames,
                                                     uint32_t batch, int32_t width,
                                                     int32_t height, int32_t stride,
                                                     int64_t frame_pitch, mage_keypoint* d_kp,
                                                     uint8_t* d_desc, uint32_t cap,
                                                     uint32_t* d_n, mage_stream stream);

/* Sticky device-side status of the batched path (capacity overflow etc.): synchronises
 * `stream` and returns MAGE_OK, MAGE_ECAPACITY or MAGE_EUNSUPPORTED; reset clears it. */
mage_status mage_orb_status(mage_orb* orb, mage_stream stream);
mage_status mage_orb_reset_status(mage_orb* orb, mage_stream stream);

/* Candidate gate of the FAST pass (no reference counterpart; a speed-only state, DESIGN.md §2
 * ORB): each batch scores exactly only the pixels that can reach a gate G derived from the
 * detector's previous batch and re-runs the exact path for frames whose retain bound lies below
 * G, so outputs never depend on it.  set: the gate of the next batch on `level` (0 = none;
 * tests and tuning).  stats: the gate the last batch used, the gate the next batch will use and
 * how many frames of the last batch took the exact path again.  Both synchronise `stream`. */
mage_status mage_orb_set_fast_gate(mage_orb* orb, uint32_t level, int32_t gate, mage_stream stream);
mage_status mage_orb_fast_gate_stats(mage_orb* orb, uint32_t level, int32_t* last_gate,
                                     int32_t* next_gate, uint32_t* last_redo, mage_stream stream);

/* Benchmark/test input generator: writes frames t0..t0+count-1 of the seeded
 * panning texture sequence, each width*height bytes at d_out + i*frame_pitch.  Identical to
 * mageslam_amd/synth.py frame(). */
mage_status mage_synth_frames_device(uint8_t* d_out, uint32_t count, int32_t width,
                                     int32_t height, int64_t frame_pitch, uint32_t t0,
                                     uint64_t seed, mage_stream stream);

/* Benchmark / test input for the tracking loop (BASELINE.json C4): `count` frames of a textured plane
 * Z = plane_z seen by a pinhole camera; d_cams holds per frame R (row-major, world -> camera) and
 * the camera centre C (12 doubles).  Texel (floor(X s) + off, floor(Y s) + off) of the panning
 * sequence's texture; identical to mageslam_amd/synth.py scene_frames(). */
mage_status mage_synth_scene_device(uint8_t* d_out, uint32_t count, int32_t width, int32_t height,
                                    int64_t frame_pitch, const double* d_cams, double fx, double fy, double cx,
                                    double cy, double plane_z, double texel_scale, int64_t texel_offset,
                                    uint64_t seed, mage_stream stream);

/* FAST-9/16 score map of FAST_t<16> with NMS disabled-equivalent view: score[y*W+x] =
 * cornerScore if (x,y) passes the segment test, else 0 (OpenCVModified.cpp:1225-1512,
 * 927-1071).  Host buffers, synchronous.  Used for the VERIFY_SIMD-style parity check. */
mage_status mage_orb_fast_score_map(const uint8_t* img, int32_t width, int32_t height,
                                    int32_t stride, int32_t threshold, uint8_t* score_map,
                                    int device);

/* Debug view of how the FAST kernels stage tile (tx, ty) (120 x 30 outputs, a 136 x 38 window from
 * (120 tx - 8, 30 ty - 4), reflect-101 outside the frame) of a width x height frame: runs on the host,
 * no device.  *path = 0 generic per-dword loop, 1 interior, 2 border.  For 1 and 2, loads holds
 * 38 x 9 pairs {byte offset in the frame, bytes loaded} (tile row major, 9 chunks per row) and, when
 * img is given, tile (38 x 136 bytes) is the window assembled from img by exactly those loads. */
mage_status mage_debug_fast_tile_plan(const uint8_t* img, int32_t width, int32_t height, int32_t stride,
                                      int32_t tx, int32_t ty, int32_t* path, int32_t* loads, uint8_t* tile);

/* Camera calibration as OrbFeatureDetector::Process receives it (Device/CameraCalibration.h):
 * the linear intrinsics of GetCameraMatrix() and the OpenCV-ordered distortion coefficients of
 * GetCVDistortionCoeffs() — K1 K2 P1 P2 K3 (Poly3k, ndist = 5) [K4 K5 K6] (Rational6k, ndist = 8);
 * ndist = 0 for DistortionType::None. */
typedef struct mage_calibration {
    float fx, fy, cx, cy;
    float dist[8];
    int32_t ndist;
} mage_calibration;

/* OrbFeatureDetector::UndistortKeypoints (OrbFeatureDetector.cpp:30-62): keypoint positions
 * through cv::undistortPoints(pts, distorted.K, distorted.dist, noArray(), undistorted.K),
 * in place.  Process() calls it only when the two calibrations differ.  Host buffers. */
mage_status mage_undistort_keypoints(const mage_calibration* distorted, const mage_calibration* undistorted,
                                     mage_keypoint* kp, uint32_t n, int device);

/* Batched device form: frame f's keypoints at d_kp + f*pitch (pitch in keypoints), d_n[f] of
 * them (e.g. the outputs of mage_orb_detect_and_compute_batch_device).  Asynchronous. */
mage_status mage_undistort_keypoints_batch_device(const mage_calibration* distorted,
                                                  const mage_calibration* undistorted, mage_keypoint* d_kp,
                                                  int64_t pitch, const uint32_t* d_n, uint32_t batch,
                                                  mage_stream stream);

/* Frame undistortion — ImagePreprocessor::UndistortImage (ImagePreprocessor.cpp:71-120).  Create
 * once per (calibration, size): CalculateUndistortedCalibration (fx, fy kept, principal point at
 * the image centre; written to *undistorted if not NULL) and cv::initUndistortRectifyMap(K, dist,
 * noArray(), K', size, CV_32FC1) on the device.  Each frame: cv::remap(INTER_LINEAR,
 * BORDER_CONSTANT 0) of a width x height 8-bit image.  ndist must be 0, 4, 5 or 8.
 * Frames arrive as GRAYSCALE8 or as the Y plane of NV12 (CreateGrayCVMat, Utils/cv.cpp:8-28): the
 * stride / pitch arguments read either layout in place. */
typedef struct mage_undistorter mage_undistorter;
mage_status mage_undistorter_create(const mage_calibration* distorted, int32_t width, int32_t height, int device,
                                    mage_undistorter** out, mage_calibration* undistorted);
mage_status mage_undistorter_destroy(mage_undistorter* u);
/* The CV_32FC1 maps (map1 = x, map2 = y), width*height floats each, for tests. */
mage_status mage_undistorter_get_maps(mage_undistorter* u, float* mapx, float* mapy);
/* Host buffers, synchronous. */
mage_status mage_undistort_image(mage_undistorter* u, const uint8_t* src, int32_t src_stride, uint8_t* dst,
                                 int32_t dst_stride);
/* Batched device form: frame f at d_src + f*src_pitch -> d_dst + f*dst_pitch.  Asynchronous. */
mage_status mage_undistort_image_batch_device(mage_undistorter* u, const uint8_t* d_src, int32_t src_stride,
                                              int64_t src_pitch, uint8_t* d_dst, int32_t dst_stride, int64_t dst_pitch,
                                              uint32_t batch, mage_stream stream);

/* cv::resize(src, dst, Size(dw, dh), 0, 0, INTER_LINEAR) for CV_8UC1 (OpenCV 3.4.0 fixed-point
 * path, the pyramid levels' resize of OpenCVModified.cpp:833), any scale.  Device buffers,
 * asynchronous on `stream`. */
mage_status mage_resize_linear_device(const uint8_t* d_src, int32_t sw, int32_t sh, int32_t src_stride, uint8_t* d_dst,
                                      int32_t dw, int32_t dh, int32_t dst_stride, mage_stream stream);

/* Stereo frame preparation — ImagePreprocessor::ScaleImageForCameraConfiguration
 * (Core/.../Source/Image/ImagePreprocessor.cpp:18-65).  A camera as the reference passes it: its
 * MAGESlam::CameraConfiguration (Extrinsics: mage::Matrix M11..M44 row-major; Size) and the
 * undistorted pinhole CameraCalibration of the same size (fx, fy, cx, cy). */
typedef struct mage_camera_config {
    float extrinsics[16];
    float fx, fy, cx, cy;
    uint32_t width, height;
} mage_camera_config;

/* The geometry: targetToSource = source.Extrinsics * inverse(target.Extrinsics) (cv::Matx44f, LU
 * inverse), the overlap crop of the source frame in the target frame at max_depth_meters
 * (CalculateOverlapCropSourceInTarget, MageUtil.cpp:13-58; crop_xywh = the cv::Rect), *ok = 0 when
 * it lies entirely offscreen (IsEntirelyOffscreen, Utils/cv.h:405-418; the reference returns
 * false), else scaleSourceToTarget and the prepared camera: size (int)(size * scale) and
 * GetScaledIntrinsics (CameraCalibration.cpp:150-157) when scale != 1, the source otherwise.
 * Host only. */
mage_status mage_scale_for_camera_configuration(const mage_camera_config* source, const mage_camera_config* target,
                                                float max_depth_meters, int32_t crop_xywh[4], float* scale,
                                                mage_camera_config* prepared, int32_t* ok);

/* CalculateOverlapCropSourceInTarget (MageUtil.cpp:13-58) from the matrix itself, the inner part of
 * the geometry above: the cv::Rect, in the target frame, of the source frame's corners at
 * depth_meters.  StereoMapInit::Initialize (Stereo/StereoMapInit.cpp:100) calls it with
 * target_to_source = frame0ToFrame1 (cv::Matx44f, row-major), target = frame 0's camera and source =
 * frame 1's to get the crop that masks frame 0's keypoints (mage_stereo_init_triangulate*'s crop).
 * The cameras' extrinsics fields are not read.  Host only. */
mage_status mage_overlap_crop_source_in_target(const float target_to_source[16], const mage_camera_config* target,
                                               const mage_camera_config* source, float depth_meters,
                                               int32_t crop_xywh[4]);

/* The whole call on a device image: the geometry above, then the source->width x source->height
 * image at d_src (src_stride) resized with INTER_LINEAR into d_dst (dst_stride; prepared->height
 * rows of prepared->width bytes; dst_capacity bytes available), or copied when scale == 1.
 * Nothing is written when *ok = 0.  Asynchronous on `stream`. */
mage_status mage_scale_image_for_camera_configuration_device(const mage_camera_config* source,
                                                             const mage_camera_config* target, float max_depth_meters,
                                                             const uint8_t* d_src, int32_t src_stride, uint8_t* d_dst,
                                                             int32_t dst_stride, int64_t dst_capacity,
                                                             mage_camera_config* prepared, float* scale, int32_t* ok,
                                                             mage_stream stream);

/* ------------------------------------------------------------------------------------------ */
/* Hamming matching — replaces FeatureMatcher (Core/.../Source/Tracking/FeatureMatcher.h)        */
/* ------------------------------------------------------------------------------------------ */

/* GetDescriptorDistance (FeatureMatcher.cpp:453-504): popcount(a ^ b) over 32 bytes. */
int32_t mage_hamming_distance(const uint8_t* a32, const uint8_t* b32);

/* Match (FeatureMatcher.cpp:61-190): masked two-way brute force with the ratio-delta test.
 * Masks may be NULL (= all true).  Host buffers, synchronous.  Output in ascending A index. */
mage_status mage_hamming_match(const uint8_t* desc_a, uint32_t n_a, const uint8_t* mask_a,
                               const uint8_t* desc_b, uint32_t n_b, const uint8_t* mask_b,
                               int32_t max_distance, int32_t min_difference, mage_dmatch* out,
                               uint32_t cap, uint32_t* n);

/* Batched device form: pair p matches A = d_desc_a + p*a_pitch (n_a[p] rows) against
 * B = d_desc_b + p*b_pitch (n_b[p] rows); no masks.  The pitches are in bytes (multiples of 16) and
 * need not be equal; b_pitch == 0 shares one B set between all pairs (d_n_b still holds one count
 * per pair).  A pair with a zero count, or with a count above 4096, reports 0.  Results per pair at
 * d_out + p*cap: d_n[p] is the number of matches found and may exceed cap; only the first cap of
 * them (ascending A index) are written, and nothing past min(d_n[p], cap) records of a pair's
 * region is touched.  d_n_a / d_n_b are device arrays of `pairs` counts.  Asynchronous on `stream`. */
mage_status mage_hamming_match_batch_device(const uint8_t* d_desc_a, int64_t a_pitch,
                                            const uint32_t* d_n_a, const uint8_t* d_desc_b,
                                            int64_t b_pitch, const uint32_t* d_n_b,
                                            uint32_t pairs, int32_t max_distance,
                                            int32_t min_difference, mage_dmatch* d_out,
                                            uint32_t cap, uint32_t* d_n, mage_stream stream);

/* RadiusMatch (FeatureMatcher.cpp:294-378, per query :386-446) against the target set's
 * KeypointSpatialIndex (KeypointSpatialIndex.cpp:46-106, replaced by an on-device band index):
 * a query matches targets with |x - qx| <= radius, |y - qy| <= radius and the same octave; best /
 * "second best" as the reference's loop visits candidates in ascending target index; accepted
 * when second - best > min_difference; then only matches whose distance is the unique minimum
 * among the matches to their target survive.  query_pos (n_query x 2 floats) overrides the query
 * positions (queryKeypointPositionOverrides); masks and query_pos may be NULL.  At most 4096
 * targets.  Host buffers, synchronous; output in query order (train_idx = target index). */
mage_status mage_radius_match(const mage_keypoint* query_kp, const float* query_pos,
                              const uint8_t* query_mask, const uint8_t* query_desc, uint32_t n_query,
                              const mage_keypoint* target_kp, const uint8_t* target_mask,
                              const uint8_t* target_desc, uint32_t n_target, float radius,
                              int32_t max_distance, int32_t min_difference, mage_dmatch* out,
                              uint32_t cap, uint32_t* n);

/* TrackLocalMap's per-map-point matching (TrackLocalMap.cpp:175-256: ProjectMapPointIntoCurrentFrame
 * -> MatchMapPointToCurrentFrame -> the single-query RadiusMatch of FeatureMatcher.cpp:386-446) over
 * projected map points in order: point i searches the frame keypoints in its box (|x - qx| <=
 * radius, |y - qy| <= radius, same octave) that are still unassociated (mask[t] != 0), keeps the best
 * Hamming distance with the reference's "second = previous best" rule (candidates in ascending
 * keypoint order) and, when best <= max_distance and second - best > min_difference, associates
 * keypoint t: result[i] = t and mask[t] = 0 for every later point.  query_hide[i] >= 0 is the
 * keypoint a pose-estimation outlier point was matched to, hidden from its own search (:192-229);
 * NULL = none.  result[i] = -1 when no match.  Host buffers, synchronous; n_target <= 4096. */
mage_status mage_local_map_match(const float* query_pos, const int32_t* query_octave, const uint8_t* query_desc,
                                 const int32_t* query_hide, uint32_t n_query, const mage_keypoint* target_kp,
                                 const uint8_t* target_desc, uint32_t n_target, uint8_t* mask, float radius,
                                 int32_t max_distance, int32_t min_difference, int32_t* result, int device);

/* Batched device form, one (query set, target set) pair per workgroup (several below 128 pairs):
 * pair p reads query_pitch / target_pitch entries further on (keypoints, positions, 32-byte
 * descriptors; the two pitches need not be equal), counts from d_n_query[p] / d_n_target[p]; no
 * masks.  d_query_pos may be NULL (the keypoints' own positions); otherwise pair p's overrides are
 * at d_query_pos + 2*p*query_pitch floats.  d_scratch: pairs x query_pitch int32.  Results at
 * d_out + p*cap: d_n[p] is the number of matches found and may exceed cap; only the first cap of
 * them (query order) are written, and nothing past min(d_n[p], cap) records of a pair's region is
 * touched.  A pair without queries reports 0 and is not checked any further; one without targets
 * reports 0.  A pair with queries whose target set exceeds 4096 ORs bit 0 into *d_status (zeroed
 * by the caller); otherwise one with a count above its pitch (n_query > query_pitch or n_target >
 * target_pitch) ORs bit 1 into it: one bit per offending pair, bit 0 taking precedence.  Such a
 * pair reports 0 matches and the other pairs are unaffected.  Asynchronous on `stream`. */
mage_status mage_radius_match_batch_device(const mage_keypoint* d_query_kp, const float* d_query_pos,
                                           const uint8_t* d_query_desc, int64_t query_pitch,
                                           const uint32_t* d_n_query, const mage_keypoint* d_target_kp,
                                           const uint8_t* d_target_desc, int64_t target_pitch,
                                           const uint32_t* d_n_target, uint32_t pairs, float radius,
                                           int32_t max_distance, int32_t min_difference,
                                           int32_t* d_scratch, mage_dmatch* d_out, uint32_t cap,
                                           uint32_t* d_n, uint32_t* d_status, mage_stream stream);

/* ------------------------------------------------------------------------------------------ */
/* Vocabulary tree + IndexedMatch — replaces OnlineBow::FindLeafNode / QueryFeatures and          */
/* IndexedMatch (Core/.../Source/BoW/OnlineBow.cpp, Tracking/FeatureMatcher.cpp:192-292)          */
/* ------------------------------------------------------------------------------------------ */

typedef struct mage_bow mage_bow;

/* The OnlineBow tree as CreateTree / Kmean build it (OnlineBow.cpp:325-411): node i has the
 * 32-byte descriptor node_desc + 32 i and children children[child_start[i] .. child_start[i+1])
 * in childrenIDs order; node 0 is the root.  Children must have larger ids than their parent
 * (Kmean appends them after it) — MAGE_EINVAL otherwise. */
mage_status mage_bow_create(const uint8_t* node_desc, const uint32_t* child_start, const uint32_t* children,
                            uint32_t n_nodes, int device, mage_bow** out);
/* OnlineBow::CreateTree (Core/MAGESLAM/Source/BoW/OnlineBow.cpp:325-337) over n training
 * descriptors (host, 32 B each): hierarchical Kmean (:451-485) with InitializeTraining's
 * std::shuffle(mt19937{}) (:396-411, MSVC STL algorithm), IterateClusteringKmean (:587-614),
 * KmeanCenter (:551-585) and FindCluster (:631-638) — the clustering iterations run on the GPU,
 * every node of a tree level at once.  levels / branching / max_iter = BagOfWordsSettings
 * TrainingTreeLevels / TrainingTreeBranchingFactor / MaxTrainingIteration (MageSettings.h:230-232;
 * branching <= 16 here).  Node ids follow the reference's recursion.  SetNodeWeights (IDF) is host
 * bookkeeping over mage_bow_find_leaves (mageslam_amd/bow.py OnlineBow). */
mage_status mage_bow_train(const uint8_t* desc, uint32_t n, uint32_t levels, uint32_t branching, uint32_t max_iter,
                           int device, mage_bow** out);
/* The same tree built by OnlineBow::Kmedoid (OnlineBow.cpp:487-521, IterateClusteringKmedoid
 * :590-639) instead of Kmean: every node is the member of its group with the first smallest sum of
 * distances to the group (an empty group keeps its medoid; the reference reads past an empty
 * vector there). */
mage_status mage_bow_train_kmedoid(const uint8_t* desc, uint32_t n, uint32_t levels, uint32_t branching,
                                   uint32_t max_iter, int device, mage_bow** out);
/* The tree of `bow` (node_desc n x 32, child_start n + 1, children n - 1); MAGE_ECAPACITY with
 * *n_nodes set when cap_nodes is too small. */
mage_status mage_bow_get_tree(mage_bow* bow, uint8_t* node_desc, uint32_t* child_start, uint32_t* children,
                              uint32_t cap_nodes, uint32_t* n_nodes);
mage_status mage_bow_destroy(mage_bow* bow);

/* FindLeafNode (OnlineBow.cpp:289-311) of n descriptors: leaf[i] = node id.  Host buffers,
 * synchronous; _device: device buffers, asynchronous on `stream`. */
mage_status mage_bow_find_leaves(mage_bow* bow, const uint8_t* desc, uint32_t n, uint32_t* leaf);
mage_status mage_bow_find_leaves_device(mage_bow* bow, const uint8_t* d_desc, uint32_t n, uint32_t* d_leaf,
                                        mage_stream stream);

/* IndexedMatch (FeatureMatcher.cpp:192-292) with the BoW candidate lists (OnlineBowFeatureMatcher::
 * QueryFeatures / OnlineBow::QueryFeatures: the other image's features in the query's leaf, in
 * index order): forward TrackMatch best / second best, accepted when best < max_distance + 1 and
 * (second >= max_distance + 1 or second - best >= min_difference); kept when the reverse match
 * of B[j] over A's features of the same leaf returns A[i] with the same test.  Masks may be NULL
 * (all true).  At most 4096 features per side.  Host buffers, synchronous; output in A order,
 * DMatch(queryIdx = A index, trainIdx = B index, imgIdx = -1, distance). */
mage_status mage_indexed_match(mage_bow* bow, const uint8_t* desc_a, uint32_t n_a, const uint8_t* mask_a,
                               const uint8_t* desc_b, uint32_t n_b, const uint8_t* mask_b, int32_t max_distance,
                               int32_t min_difference, mage_dmatch* out, uint32_t cap, uint32_t* n);

/* Batched device form, one (A, B) pair per workgroup, leaves precomputed (e.g. by
 * mage_bow_find_leaves_device): pair p reads a_pitch / b_pitch entries further on (descriptors,
 * leaves, optional masks; either mask may be NULL on its own, the pitches need not be equal), counts
 * d_n_a[p] / d_n_b[p]; a pair with a zero (masked) count on either side reports 0.  Results at
 * d_out + p*cap: d_n[p] is the number of matches found and may exceed cap; only the first cap of
 * them (ascending A index) are written, and nothing past min(d_n[p], cap) records of a pair's
 * region is touched.  Bit 0 of *d_status (zeroed by the caller) is set when a side exceeds 4096;
 * that pair reports 0 and the other pairs are unaffected.  Asynchronous. */
mage_status mage_indexed_match_batch_device(const uint8_t* d_desc_a, const uint32_t* d_leaf_a, const uint8_t* d_mask_a,
                                            int64_t a_pitch, const uint32_t* d_n_a, const uint8_t* d_desc_b,
                                            const uint32_t* d_leaf_b, const uint8_t* d_mask_b, int64_t b_pitch,
                                            const uint32_t* d_n_b, uint32_t pairs, int32_t max_distance,
                                            int32_t min_difference, mage_dmatch* d_out, uint32_t cap, uint32_t* d_n,
                                            uint32_t* d_status, mage_stream stream);

/* ------------------------------------------------------------------------------------------ */
/* New map points — replaces NewMapPointsCreation's CreateInitialAssociations                  */
/* (Core/.../Source/Mapping/NewMapPointsCreation.cpp)                                          */
/* ------------------------------------------------------------------------------------------ */

/* NewMapPointsCreationSettings (MageSettings.h:55-61), the pyramid of Ki, and the grid cap of
 * CameraSettings (MageSettings.h:311-313).  struct_size must be sizeof(mage_new_points_settings);
 * anything else is MAGE_EINVAL. */
typedef struct mage_new_points_settings {
    uint32_t struct_size;
    float max_epipolar_error;          /* 3.84385518580709 (pixels) */
    float min_accepted_distance_ratio; /* 2.0 */
    float min_parallax_degrees;        /* 0.0238961594253207 */
    float pyramid_scale;               /* Ki's pyramid scale factor (> 1) */
    uint32_t num_levels;               /* Ki's pyramid levels, 1..MAGE_MAX_LEVELS */
    uint32_t grid_width;               /* NewPointGridWidth 4 */
    uint32_t grid_height;              /* NewPointGridHeight 3 (at most 64 cells) */
    uint32_t max_grid_count;           /* NewPointMaxGridCount 6 */
    uint32_t image_width, image_height;
} mage_new_points_settings;

/* One created map point, in the order of the reference's newMapPoints.push_back (:156): position,
 * proxy::ViewingData {mean view direction, dMin, dMax} and the two associations (Ki keypoint; Kc
 * slot and keypoint), plus the match's index within its slot.  48 bytes. */
typedef struct mage_new_point {
    float position[3];
    float mean_view_dir[3];
    float d_min, d_max;
    uint32_t ki_index, kc_slot, kc_index, match_index;
} mage_new_point;

/* Verdict of a match: the reference's first reason to drop it, in the reference's order. */
#define MAGE_NP_ACCEPTED 0
#define MAGE_NP_EPIPOLAR 1       /* both epipolar distances sum over 2 * MaxEpipolarError (:82-88) */
#define MAGE_NP_BEHIND 2         /* VerifyProjectInFront of Ki, then Kc (:96-100) */
#define MAGE_NP_DISTANCE_RATIO 3 /* |X - Ci| / |Ci - Cc| < MinAcceptedDistanceRatio (:117-123) */
#define MAGE_NP_SCALE 4          /* predicted octave differs from the Kc keypoint's (:126-130) */
#define MAGE_NP_PARALLAX 5       /* cos of the two viewing directions > CosMinParallax (:137) */
#define MAGE_NP_GRID_FULL 6      /* the Ki keypoint's grid cell is full at the match's turn (:301) */
#define MAGE_NP_KI_TAKEN 7       /* an earlier match made a point of this Ki keypoint (:309) */
#define MAGE_NP_BAD_INDEX 8      /* queryIdx / trainIdx or a keypoint octave out of range: nothing read */

/* CreateInitialAssociations' loop over the matches of up to 8 covisible keyframes Kc against the new
 * keyframe Ki (NewMapPointsCreation.cpp:171-329 from the grid counts on; the per-match geometry is
 * TryCreateNewAssociatedMapPointForMatch, :74-160, with ComputeFundamentalMatrix, Utils/Epipolar.cpp:
 * 14-48, DistanceFromEpipolarLine, :94-107, TriangulatePointWorldSpace, Tracking/Triangulation.cpp:
 * 24-60, and ComputeOctave / ComputeDMin / ComputeDMax, Map/MappingMath.h:13-40).  Poses as
 * mage_ba_set_cameras takes them: pos3 the view-space t, r9 the column-major R, intr4 {cx, cy, fx,
 * fy}.  ki_associated (n_ki bytes, NULL = none) is Ki's associated-keypoint mask, which seeds the
 * grid counts (:187-201).  The Kc slots are in processing order; their keypoints and their matches
 * (queryIdx = Kc keypoint, trainIdx = Ki keypoint, as IndexedMatch(Kc, Ki) returns them) are
 * concatenated, slot k owning [start[k], start[k + 1]).  verdict gets one MAGE_NP_* per match;
 * accepted points go to out[0 .. min(*n_out, cap)) in processing order.  *status: bit 0 when n_ki
 * exceeds 4096 (no points, verdicts untouched), bit 1 when more than cap points were accepted
 * (*n_out is then cap).  More than 8 slots, more than 8 levels or more than 64 grid cells is
 * MAGE_EINVAL.  Host buffers, synchronous, runs on `device`. */
mage_status mage_new_map_points(const mage_new_points_settings* settings, const float* ki_pos3, const float* ki_r9,
                                const float* ki_intr4, const mage_keypoint* ki_kp, uint32_t n_ki,
                                const uint8_t* ki_associated, uint32_t n_kc, const float* kc_pos3, const float* kc_r9,
                                const float* kc_intr4, const mage_keypoint* kc_kp, const uint32_t* kc_kp_start,
                                const mage_dmatch* matches, const uint32_t* match_start, mage_new_point* out,
                                uint32_t cap, uint32_t* n_out, uint8_t* verdict, uint32_t* status, int device);

/* The same in plain C++ on the calling thread, with the reference's sequential loop (:290-321)
 * over the same per-match arithmetic: the CPU backend, bit-identical to the kernel.  No GPU. */
mage_status mage_new_map_points_host(const mage_new_points_settings* settings, const float* ki_pos3,
                                     const float* ki_r9, const float* ki_intr4, const mage_keypoint* ki_kp,
                                     uint32_t n_ki, const uint8_t* ki_associated, uint32_t n_kc, const float* kc_pos3,
                                     const float* kc_r9, const float* kc_intr4, const mage_keypoint* kc_kp,
                                     const uint32_t* kc_kp_start, const mage_dmatch* matches,
                                     const uint32_t* match_start, mage_new_point* out, uint32_t cap, uint32_t* n_out,
                                     uint8_t* verdict, uint32_t* status);

/* Batched device form, one workgroup per problem (one Ki with d_n_kc[problem] <= kc_slots <= 8 Kc
 * slots); pair = problem * kc_slots + slot.  Ki arrays advance per problem (poses 3 / 9 / 4 floats,
 * keypoints and the optional associated mask ki_pitch entries, count d_n_ki[problem]); Kc arrays
 * advance per pair (keypoints kc_pitch entries, count d_n_kc_kp[pair]).  The matches are read in
 * the layout mage_indexed_match_batch_device writes with A = Kc and B = Ki: d_matches + pair *
 * match_cap, count d_n_matches[pair] (a count over match_cap reads match_cap), so the two launches
 * chain on one stream.  Verdicts at d_verdict + pair * match_cap, points at d_out + problem * cap,
 * count in d_n_out[problem].  Bits of *d_status as above; bit 0 also for a problem with more than
 * kc_slots slots or a Kc keypoint count over kc_pitch (that problem reports 0 points).
 * Asynchronous on `stream`. */
mage_status mage_new_map_points_batch_device(const mage_new_points_settings* settings, uint32_t problems,
                                             uint32_t kc_slots, const float* d_ki_pos3, const float* d_ki_r9,
                                             const float* d_ki_intr4, const mage_keypoint* d_ki_kp, int64_t ki_pitch,
                                             const uint32_t* d_n_ki, const uint8_t* d_ki_associated,
                                             const uint32_t* d_n_kc, const float* d_kc_pos3, const float* d_kc_r9,
                                             const float* d_kc_intr4, const mage_keypoint* d_kc_kp, int64_t kc_pitch,
                                             const uint32_t* d_n_kc_kp, const mage_dmatch* d_matches,
                                             uint32_t match_cap, const uint32_t* d_n_matches, mage_new_point* d_out,
                                             uint32_t cap, uint32_t* d_n_out, uint8_t* d_verdict, uint32_t* d_status,
                                             mage_stream stream);

/* LocallyAssociateNewAssociations (NewMapPointsCreation.cpp:337-424): the second half of
 * NewMapPointsCreation.  NewMapPointsCreationSettings' association part (MageSettings.h:55-61) and
 * Ki's image border; mage_new_points_settings supplies pyramid_scale, num_levels and the image
 * size, which is taken for every keyframe (one camera; the reference reads each keyframe's own
 * size — stereo pairs with differing sizes are not covered).  struct_size must be
 * sizeof(mage_new_points_assoc_settings); anything else is MAGE_EINVAL. */
typedef struct mage_new_points_assoc_settings {
    uint32_t struct_size;
    float search_radius;              /* NewMapPointsSearchRadius 11.8816156 (pixels) */
    float max_keyframe_angle_degrees; /* MaxKeyframeAngleDegrees 60 */
    float image_border;               /* Ki's GetImageBorder(); the gate uses border - radius / 2 (:345) */
    int32_t max_hamming_distance;     /* AssociateMatcherSettings.MaxHammingDistance 30, in [-1, 256] */
    int32_t min_hamming_difference;   /* AssociateMatcherSettings.MinHammingDifference 1 */
} mage_new_points_assoc_settings;

/* What one new point found in one keyframe: the projection (ProjectUndistorted), the predicted
 * octave and the keypoint it was associated with, or -1.  A field the reference had not computed
 * when it skipped or refused the pair is 0 (x, y, octave) or -1 (keypoint): x and y are 0 for
 * SAME_FRAME and BAD_INDEX (nothing projected), octave is 0 up to and including DISTANCE.
 * 16 bytes. */
typedef struct mage_new_point_assoc {
    float x, y;
    int32_t octave;
    int32_t keypoint;
} mage_new_point_assoc;

/* Verdict of a (point, keyframe) pair: the reference's first reason, in the reference's order. */
#define MAGE_NA_ASSOCIATED 0 /* Keyframes.push_back + SetKeypointAsAssociated (:408-409) */
#define MAGE_NA_SAME_FRAME 1 /* the point already has an association with this keyframe (:366-369) */
#define MAGE_NA_BEHIND 2     /* IsGoodCandidate: depth < 0 (TrackLocalMap.cpp:529) */
#define MAGE_NA_BORDER 3     /* IsGoodCandidate: outside the image less the border (:529) */
#define MAGE_NA_ANGLE 4      /* IsGoodCandidate: mean view direction . forward < cos(max angle) (:541) */
#define MAGE_NA_DISTANCE 5   /* IsGoodCandidate: outside [dMin, dMax] (:549) */
#define MAGE_NA_OCTAVE 6     /* predicted octave < 0 or > numLevels (:392; the test is >, not >=) */
#define MAGE_NA_NO_MATCH 7   /* MatchMapPointToCurrentFrame found nothing (:399) */
#define MAGE_NA_BAD_INDEX 8  /* ki_index >= n_ki, kc_slot >= 8, or kc_index beyond its keyframe: nothing read */

/* The loop of LocallyAssociateNewAssociations over the points mage_new_map_points wrote (outer, in
 * push_back order) and ALL covisible keyframes (inner, in the order CreateInitialAssociations'
 * std::sort left, :217): a keyframe the point is already associated with is skipped; the point is
 * projected (ProjectUndistorted, Tracking/Reprojection.cpp:26-42), gated (TrackLocalMap::
 * IsGoodCandidate, TrackLocalMap.cpp:519-554, border = image_border - search_radius / 2) and given
 * an octave (ComputeOctave), then matched by the single-query RadiusMatch (FeatureMatcher.cpp:
 * 386-446; box, octave, availability and best / second rules as mage_local_map_match) with Ki's
 * descriptor at the point's ki_index against the keyframe's still-unassociated keypoints; a success
 * takes the keypoint for every later point.
 * Keyframe k: pose and calibration as above, keypoints, 32-byte descriptors and mask bytes
 * concatenated, keyframe k owning [kf_start[k], kf_start[k + 1]).  kf_slot[k] is the Kc slot the
 * keyframe had in mage_new_map_points, or -1 (in [-1, 7]).  kf_mask is in/out: on entry byte t != 0
 * means keypoint t was unassociated when IndexedMatch ran; the entry first clears, in keyframe k's
 * mask, kc_index of every point with kc_slot == kf_slot[k] (CreateInitialAssociations' own
 * SetKeypointAsAssociated, :314), then runs the loop; on return the taken keypoints are 0 too.
 * A point with kc_slot == kf_slot[k] is SAME_FRAME for keyframe k (BAD_INDEX when its kc_index is
 * not a keypoint of k); a point with ki_index >= n_ki or kc_slot >= 8 is BAD_INDEX everywhere.
 * Outputs are point-major: out[p * n_kf + k], verdict[p * n_kf + k].  *status bit 0: a keyframe has
 * more than 4096 keypoints — its verdict bytes are left untouched, its records are {0, 0, 0, -1},
 * its mask is unchanged, the other keyframes are unaffected.  n_points == 0 or n_kf == 0 returns
 * MAGE_OK with nothing written.  No limit on n_kf.  Host buffers, synchronous, runs on `device`. */
mage_status mage_new_points_associate(const mage_new_points_settings* settings,
                                      const mage_new_points_assoc_settings* assoc, const mage_new_point* points,
                                      uint32_t n_points, const uint8_t* ki_desc, uint32_t n_ki, uint32_t n_kf,
                                      const float* kf_pos3, const float* kf_r9, const float* kf_intr4,
                                      const mage_keypoint* kf_kp, const uint8_t* kf_desc, const uint32_t* kf_start,
                                      const int32_t* kf_slot, uint8_t* kf_mask, mage_new_point_assoc* out,
                                      uint8_t* verdict, uint32_t* status, int device);

/* The same in plain C++ on the calling thread, with the reference's literal nested loop (points
 * outer, keyframes inner, the mask updated as it goes): the CPU backend, bit-identical to the
 * kernel.  No GPU. */
mage_status mage_new_points_associate_host(const mage_new_points_settings* settings,
                                           const mage_new_points_assoc_settings* assoc, const mage_new_point* points,
                                           uint32_t n_points, const uint8_t* ki_desc, uint32_t n_ki, uint32_t n_kf,
                                           const float* kf_pos3, const float* kf_r9, const float* kf_intr4,
                                           const mage_keypoint* kf_kp, const uint8_t* kf_desc,
                                           const uint32_t* kf_start, const int32_t* kf_slot, uint8_t* kf_mask,
                                           mage_new_point_assoc* out, uint8_t* verdict, uint32_t* status);

/* Batched device form, one workgroup per pair = problem * kf_slots + k.  The points are read as
 * mage_new_map_points_batch_device leaves them: d_points + problem * cap, count d_n_points[problem]
 * (a count over cap reads cap).  Ki's descriptors advance by ki_pitch per problem (count
 * d_n_ki[problem]); keyframe arrays advance per pair (poses 3 / 9 / 4 floats; keypoints,
 * descriptors and mask bytes kf_pitch entries, count d_n_kf_kp[pair]); problem i uses its first
 * d_n_kf[i] pairs, d_kf_slot[pair] as kf_slot above.  Records at d_assoc + (problem * cap + p) *
 * kf_slots + k, verdicts likewise; nothing is written beyond the counts.  The masks are device
 * bytes, in/out.  Bit 0 of *d_status as above, and also for d_n_kf[problem] > kf_slots (every pair of
 * that problem is treated as over the limit) or a keypoint count over kf_pitch.  Descriptor
 * pointers must be 16-byte aligned.  Asynchronous on `stream`: find_leaves, indexed_match_batch,
 * new_map_points_batch and this entry chain on one stream with no host step. */
mage_status mage_new_points_associate_batch_device(const mage_new_points_settings* settings,
                                                   const mage_new_points_assoc_settings* assoc, uint32_t problems,
                                                   uint32_t kf_slots, const mage_new_point* d_points, uint32_t cap,
                                                   const uint32_t* d_n_points, const uint8_t* d_ki_desc,
                                                   int64_t ki_pitch, const uint32_t* d_n_ki, const uint32_t* d_n_kf,
                                                   const float* d_kf_pos3, const float* d_kf_r9,
                                                   const float* d_kf_intr4, const mage_keypoint* d_kf_kp,
                                                   const uint8_t* d_kf_desc, uint8_t* d_kf_mask, int64_t kf_pitch,
                                                   const uint32_t* d_n_kf_kp, const int32_t* d_kf_slot,
                                                   mage_new_point_assoc* d_assoc, uint8_t* d_verdict,
                                                   uint32_t* d_status, mage_stream stream);

/* ------------------------------------------------------------------------------------------ */
/* Cheap loop closure — the map-point refresh after an association                              */
/* (Core/.../Source/Map/MapPoint.cpp:35-46, 80-155)                                            */
/* ------------------------------------------------------------------------------------------ */

/* What the mapping task's CheapLoopClosure (Tasks/MappingWorker.cpp:20-73) and TryConnectMapPoints
 * (Map/ThreadSafeMap.cpp:715-787) read of the settings: LoopClosureSettings (MageSettings.h:197-207),
 * TrackLocalMapSettings' view angle and matcher (:180-194), the keyframe's image border and size and
 * the pyramid.  struct_size must be sizeof(mage_loop_closure_settings); anything else is
 * MAGE_EINVAL.  The refresh entries below read num_levels and pyramid_scale; the other fields are
 * checked and belong to the closure and connect steps. */
typedef struct mage_loop_closure_settings {
    uint32_t struct_size;
    uint32_t max_map_points;  /* LoopClosureSettings.MaxMapPoints 200, in 1..1024 */
    uint32_t min_keyframes;   /* LoopClosureSettings.MinKeyframe 10 */
    float search_radius;      /* LoopClosureSettings.MatchSearchRadius 18 (pixels), >= 0 */
    float min_view_degrees;   /* TrackLocalMapSettings.MinDegreesBetweenCurrentViewAndMapPointView 60 */
    float image_border;       /* GetImageBorder(); the gate uses border - search_radius / 2 (MappingWorker.cpp:45) */
    uint32_t width, height;   /* image size, positive */
    uint32_t num_levels;      /* pyramid levels, in 1..8 */
    float pyramid_scale;      /* pyramid scale, > 1 */
    int32_t closure_max_hamming_distance;   /* CheapLoopClosureMatchingSettings.MaxHammingDistance 30, in [-1, 256] */
    int32_t closure_min_hamming_difference; /* CheapLoopClosureMatchingSettings.MinHammingDifference 1 */
    int32_t connect_max_hamming_distance;   /* TrackLocalMapSettings.OrbMatcherSettings.MaxHammingDistance 30 */
    int32_t connect_min_hamming_difference; /* TrackLocalMapSettings.OrbMatcherSettings.MinHammingDifference 1 */
} mage_loop_closure_settings;

/* One observation of a map point: what MapPoint's refresh reads of the observing keyframe.  The
 * descriptor comes first and the record is 16-byte aligned, so a device list of them can be read
 * with 16-byte loads.  64 bytes. */
typedef struct mage_map_point_obs {
    uint8_t desc[32];    /* the associated keypoint's descriptor */
    float centre[3];     /* the keyframe's GetWorldSpacePosition() */
    int32_t octave;      /* the associated keypoint's octave */
    int32_t keyframe_id; /* carried, not read */
    uint32_t reserved[3];
} mage_map_point_obs;

/* A map point's derived state.  rep is the index, in the point's observation list, of
 * m_representativeDescriptorKeyframe, or -1 for a point without observations.  40 bytes. */
typedef struct mage_map_point_state {
    float pos[3];  /* m_position */
    float mvd[3];  /* m_meanViewingDirection */
    float dmin, dmax;
    int32_t rep;
    int32_t n_obs;
} mage_map_point_state;

#define MAGE_MP_MAX_OBS 65536 /* observations of one point: the summed distance stays exact in float */

/* MapPoint::UpdateRepresentativeDescriptor and UpdateMeanViewDirectionAndDistances (MapPoint.cpp:
 * 80-155) for n_points points, as AddKeyframeAssociation (:35-46) runs them after every new
 * association.  Point i has position positions[3 i .. 3 i + 2] and observations obs[i * obs_pitch ..
 * i * obs_pitch + n_obs[i]), in the order of m_keyframes.
 *   rep   -1 for no observation; otherwise the observation with the first strictly smallest sum of
 *         Hamming distances to all of the point's observations, itself included (:105-125; the
 *         reference sums in float, which is exact below 65536 observations).
 *   mvd   {0, 0, 0} for no observation; otherwise Normalize of the sum, from {0, 0, 0} and in
 *         observation order, of Normalize(pos - centre) (:141-146).  Normalize as Utils/cv.h:
 *         287-296: a zero-length vector is left as it is; the norm is sqrtf of the float dot
 *         product and the division multiplies by the float reciprocal, as the tracker's
 *         one-keyframe case does.
 *   dmax, dmin   |centre_rep - pos| times ComputeDMax's / ComputeDMin's factor of the representative
 *         keypoint's octave (Map/MappingMath.h:32-40; the octave is clamped to the tables' 0..7).
 *         0 for no observation (the reference keeps the values it had).
 * state[i] also gets pos and n_obs.  obs_pitch must be in 1..MAGE_MP_MAX_OBS and no n_obs[i] may
 * exceed it (MAGE_EINVAL, nothing written).  n_points == 0 returns MAGE_OK.  Plain C++ on the
 * calling thread: the CPU backend, bit-identical to the kernel.  No GPU. */
mage_status mage_map_points_refresh_host(const mage_loop_closure_settings* settings, uint32_t n_points,
                                         const float* positions, const mage_map_point_obs* obs, int64_t obs_pitch,
                                         const uint32_t* n_obs, mage_map_point_state* state);

/* The same on the GPU.  Host buffers, synchronous, runs on `device`. */
mage_status mage_map_points_refresh(const mage_loop_closure_settings* settings, uint32_t n_points,
                                    const float* positions, const mage_map_point_obs* obs, int64_t obs_pitch,
                                    const uint32_t* n_obs, mage_map_point_state* state, int device);

/* Device buffers, one wave per point, asynchronous on `stream`.  d_obs must be 16-byte aligned.  A
 * point whose count exceeds obs_pitch sets bit 0 of *d_status and its state is left untouched; the
 * other points are unaffected.  *d_status is only ever ORed into. */
mage_status mage_map_points_refresh_batch_device(const mage_loop_closure_settings* settings, uint32_t n_points,
                                                 const float* d_positions, const mage_map_point_obs* d_obs,
                                                 int64_t obs_pitch, const uint32_t* d_n_obs,
                                                 mage_map_point_state* d_state, uint32_t* d_status,
                                                 mage_stream stream);

/* What one sampled point found in one keyframe: the projection (ProjectUndistorted), the predicted
 * octave and the keypoint it was associated with, or -1.  A field the reference had not computed
 * when it skipped or refused the pair is 0 (x, y, octave) or -1 (keypoint), by the rule of
 * mage_new_point_assoc: x and y are 0 for NOT_SAMPLED and HAS_POINT, octave is 0 up to and
 * including DISTANCE.  16 bytes. */
typedef struct mage_loop_closure_assoc {
    float x, y;
    int32_t octave;
    int32_t keypoint;
} mage_loop_closure_assoc;

/* Verdict of a (sampled point, keyframe) pair: the reference's first reason, in its order. */
#define MAGE_LC_ASSOCIATED 0  /* extraAssociations.emplace_back (MappingWorker.cpp:67, ThreadSafeMap.cpp:764) */
#define MAGE_LC_NOT_SAMPLED 1 /* connect stage: the closure did not associate the point, so TryConnectMapPoints is not given it */
#define MAGE_LC_HAS_POINT 2   /* HasMapPoint / IsAssociatedToMapPoint (MappingWorker.cpp:51, ThreadSafeMap.cpp:752) */
#define MAGE_LC_BEHIND 3      /* IsGoodCandidate: depth < 0 (TrackLocalMap.cpp:529) */
#define MAGE_LC_BORDER 4      /* IsGoodCandidate: outside the image less the border (:529) */
#define MAGE_LC_ANGLE 5       /* IsGoodCandidate: mean view direction . forward < cos(min view degrees) (:541) */
#define MAGE_LC_DISTANCE 6    /* IsGoodCandidate: outside [dMin, dMax] (:549) */
#define MAGE_LC_OCTAVE 7      /* predicted octave < 0 or > numLevels (:365; the test is >, not >=) */
#define MAGE_LC_NO_MATCH 8    /* MatchMapPointToCurrentFrame found nothing (:375), or the point has no descriptor */

#define MAGE_LC_STATUS_OVER_LIMIT 1u /* a keyframe has more than 4096 keypoints (batch form: or exceeds its pitch / slots) */
#define MAGE_LC_STATUS_OBS_FULL 2u   /* a sampled point's observation list cannot hold n_obs + 1 + n_kf entries */

/* One mapping task's CheapLoopClosure (Tasks/MappingWorker.cpp:20-73), InsertKeyframe's effect on
 * the points it associated (Map/ThreadSafeMap.cpp:242-249, MapPoint.cpp:35-46) and
 * TryConnectMapPoints (ThreadSafeMap.cpp:715-787), MappingWorker.cpp:160-181.
 *
 * The map: n_map points in map order, state[i] and the observation list obs[i * obs_pitch ..
 * + state[i].n_obs) of each, both in/out; a point's descriptor is that of observation state[i].rep.
 * Sampling (Map/Map.cpp:319-333): step = n_map / max_map_points + 1 in uint32, point i is sampled
 * iff (offset + i + 1) % step == 0 with uint32 wrap, offset the mapping task's frame counter; the
 * sample is cut at max_map_points.  n_keyframes is the map's keyframe count (:22).
 *
 * The new keyframe Ki: ki_id, pose and calibration as mage_new_points_associate takes them (pos3
 * the view-space t, r9 the column-major R, intr4 {cx, cy, fx, fy}), n_ki keypoints with 32-byte
 * descriptors, and ki_point[t] = the map-point index keypoint t is associated with, or -1: the
 * unassociated mask is ki_point < 0, HasMapPoint(i) is "i appears in ki_point".  The n_kf
 * covisible keyframes, in the order GetCovisibilityConnectedKeyframes gives them, have the same
 * fields concatenated, keyframe k owning [kf_start[k], kf_start[k + 1]), their ids kf_id and their
 * unassociated mask bytes kf_mask, in/out (byte != 0: available).
 *
 * Closure: the sampled points are offered to Ki in order; a point Ki holds is HAS_POINT; the rest go
 * through ProjectMapPointIntoCurrentFrame (TrackLocalMap.cpp:325-388: ProjectUndistorted,
 * IsGoodCandidate :519-554 with border = image_border - search_radius / 2 and the angle
 * min_view_degrees, ComputeOctave, then the single-query RadiusMatch of search_radius under the
 * closure matcher pair); a success takes the keypoint for every later point.  Every associated point
 * then gains {Ki's descriptor and octave at the keypoint, Ki's centre, ki_id} as its last
 * observation and is refreshed as mage_map_points_refresh does.
 * Connect: the covisible keyframes are visited in order; in each, the points the closure associated
 * are visited in order, a point the keyframe holds is HAS_POINT, the others go through
 * ProjectMapPointIntoCurrentFrame with their CURRENT state under the connect matcher pair, successes
 * clearing the keyframe's mask as they happen; after the keyframe's loop each success is appended
 * to its point's observations and the point refreshed, before the next keyframe is visited.
 *
 * Outputs, j the place in the sample: sample_index[j] the map index; closure[j] and
 * closure_verdict[j]; connect[j * n_kf + k] and connect_verdict[j * n_kf + k] (NOT_SAMPLED for a
 * point the closure did not associate); ki_mask[t] Ki's mask after the closure (n_ki bytes, out);
 * kf_modified[k] whether keyframe k gained an association (UpdateGraph is the caller's);
 * counts = {sampled, associated by the closure, associated by the connect stage}.
 * *status: MAGE_LC_STATUS_OVER_LIMIT when a keyframe has more than 4096 keypoints — that keyframe
 * is left untouched (its verdict bytes and mask unchanged, its records {0, 0, 0, -1}, no
 * association), the others unaffected; MAGE_LC_STATUS_OBS_FULL when obs_pitch cannot hold
 * n_obs + 1 + n_kf observations for some sampled point — the problem is refused whole before
 * anything but counts (zero) and status is written, and the synchronous forms return
 * MAGE_ECAPACITY.  n_keyframes < min_keyframes gives zero counts and writes nothing else.
 * n_kf == 0 runs the closure alone.  struct_size must be sizeof(mage_loop_closure_problem). */
typedef struct mage_loop_closure_problem {
    uint32_t struct_size;
    uint32_t n_map;
    mage_map_point_state* state;
    mage_map_point_obs* obs;
    int64_t obs_pitch;
    uint32_t offset;
    uint32_t n_keyframes;
    int32_t ki_id;
    uint32_t n_ki;
    const float *ki_pos3, *ki_r9, *ki_intr4;
    const mage_keypoint* ki_kp;
    const uint8_t* ki_desc;
    const int32_t* ki_point;
    uint32_t n_kf;
    uint32_t reserved;
    const int32_t* kf_id;
    const float *kf_pos3, *kf_r9, *kf_intr4;
    const mage_keypoint* kf_kp;
    const uint8_t* kf_desc;
    const int32_t* kf_point;
    const uint32_t* kf_start;
    uint8_t* kf_mask;
    uint32_t* sample_index;            /* max_map_points */
    mage_loop_closure_assoc* closure;  /* max_map_points */
    uint8_t* closure_verdict;          /* max_map_points */
    mage_loop_closure_assoc* connect;  /* max_map_points * n_kf */
    uint8_t* connect_verdict;          /* max_map_points * n_kf */
    uint8_t* ki_mask;                  /* n_ki */
    uint8_t* kf_modified;              /* n_kf */
    uint32_t* counts;                  /* 3 */
    uint32_t* status;                  /* 1 */
} mage_loop_closure_problem;

/* Plain C++ on the calling thread, the reference's literal nested loops: the CPU backend,
 * bit-identical to the kernels.  No GPU. */
mage_status mage_cheap_loop_closure_host(const mage_loop_closure_settings* settings,
                                         const mage_loop_closure_problem* problem);

/* The same on the GPU.  Host buffers, synchronous, runs on `device`. */
mage_status mage_cheap_loop_closure(const mage_loop_closure_settings* settings,
                                    const mage_loop_closure_problem* problem, int device);

/* Batched device form: `problems` independent mapping tasks, three launches chained on `stream`
 * (closure, its refresh, connect) with no host step.  Map arrays advance by map_pitch points
 * (observations by map_pitch * obs_pitch) per problem, Ki arrays by ki_pitch keypoints (poses 3 / 9
 * / 4 floats), covisible keyframe arrays per pair = problem * kf_slots + k by kf_pitch keypoints;
 * problem i uses its first d_n_kf[i] pairs.  Per problem: d_sample_index, d_closure and
 * d_closure_verdict at problem * max_map_points, d_connect and d_connect_verdict at ((problem *
 * max_map_points) + j) * kf_slots + k, d_ki_mask at problem * ki_pitch, d_kf_modified at pair,
 * d_counts at problem * 3, d_status at problem.  Nothing is written beyond the counts.
 * MAGE_LC_STATUS_OVER_LIMIT also for a keypoint count over its pitch; a problem with n_map >
 * map_pitch or d_n_kf > kf_slots is refused whole with that bit (zero counts).  Descriptor and
 * observation pointers must be 16-byte aligned.  struct_size must be
 * sizeof(mage_loop_closure_batch). */
typedef struct mage_loop_closure_batch {
    uint32_t struct_size;
    uint32_t problems;
    uint32_t kf_slots;
    uint32_t reserved;
    int64_t map_pitch, obs_pitch, ki_pitch, kf_pitch;
    const uint32_t* d_n_map;
    mage_map_point_state* d_state;
    mage_map_point_obs* d_obs;
    const uint32_t* d_offset;
    const uint32_t* d_n_keyframes;
    const int32_t* d_ki_id;
    const uint32_t* d_n_ki;
    const float *d_ki_pos3, *d_ki_r9, *d_ki_intr4;
    const mage_keypoint* d_ki_kp;
    const uint8_t* d_ki_desc;
    const int32_t* d_ki_point;
    const uint32_t* d_n_kf;
    const int32_t* d_kf_id;
    const float *d_kf_pos3, *d_kf_r9, *d_kf_intr4;
    const mage_keypoint* d_kf_kp;
    const uint8_t* d_kf_desc;
    const int32_t* d_kf_point;
    const uint32_t* d_n_kf_kp;
    uint8_t* d_kf_mask;
    uint32_t* d_sample_index;
    mage_loop_closure_assoc* d_closure;
    uint8_t* d_closure_verdict;
    mage_loop_closure_assoc* d_connect;
    uint8_t* d_connect_verdict;
    uint8_t* d_ki_mask;
    uint8_t* d_kf_modified;
    uint32_t* d_counts;
    uint32_t* d_status;
} mage_loop_closure_batch;

mage_status mage_cheap_loop_closure_batch_device(const mage_loop_closure_settings* settings,
                                                 const mage_loop_closure_batch* batch, mage_stream stream);

/* ------------------------------------------------------------------------------------------ */
/* Stereo map initialisation — the device stage of StereoMapInit::Initialize                   */
/* (Core/.../Source/Stereo/StereoMapInit.cpp:97-194)                                           */
/* ------------------------------------------------------------------------------------------ */

/* StereoMapInitializationSettings (MageSettings.h:135-147) in the reference's order: its nine
 * scalars, then its OrbMatcherSettings bag (:36-39) and its BundleAdjustSettings bag (:41-52).
 * struct_size must be sizeof(mage_stereo_init_settings); anything else is MAGE_EINVAL.  The device
 * stage reads max_epipolar_error, min_accepted_distance_ratio and the matcher's two; the others
 * belong to Initialize's host part (match and point counts, tether, bundle adjustment, validation). */
typedef struct mage_stereo_init_settings {
    uint32_t struct_size;
    uint32_t min_init_map_points;          /* MinInitMapPoints 15 */
    uint32_t min_feature_matches;          /* MinFeatureMatches 40 */
    float max_outlier_error;               /* MaxOutlierError 2.5 (Initialize never reads it) */
    float max_epipolar_error;              /* MaxEpipolarError 5.5 (pixels) */
    float min_accepted_distance_ratio;     /* MinAcceptedDistanceRatio 2.0 */
    float initialization_tether_strength;  /* InitializationTetherStrength 50 */
    float max_pose_contribution_z;         /* MaxPoseContributionZ 0.10 */
    float amount_ba_can_change_pose;       /* AmountBACanChangePose 1.65 */
    float max_depth_meters;                /* MaxDepthMeters 2.3 */
    int32_t max_hamming_distance;          /* OrbMatcherSettings.MaxHammingDistance 30, in [-1, 256] */
    int32_t min_hamming_difference;        /* OrbMatcherSettings.MinHammingDifference 1 */
    uint32_t ba_num_steps;                 /* BundleAdjustSettings.NumSteps 1 */
    uint32_t ba_num_steps_per_run;         /* NumStepsPerRun 1 */
    uint32_t ba_min_steps;                 /* MinSteps 1 */
    float ba_huber_width;                  /* HuberWidth 1.8 */
    float ba_huber_width_scale;            /* HuberWidthScale 0.95 */
    float ba_max_outlier_error;            /* MaxOutlierError 7.25 */
    float ba_max_outlier_error_scale_factor; /* MaxOutlierErrorScaleFactor 0.95 */
    float ba_min_mean_square_error;        /* MinMeanSquareError 0.25 */
    float ba_distance_tether_weight;       /* DistanceTetherWeight 50 */
    float ba_low_connectivity_iterations_scale; /* LowConnectivityIterationsScale 1.5 */
} mage_stereo_init_settings;

/* One accepted match, as TriangulatePoints' initial3DPoints.emplace_back(match, point) keeps it
 * (MapInitialization.cpp:984): the DMatch's indices and distance, the triangulated point, and
 * whether TriangulatePointWorldSpace took its near-parallel branch (D < 0.00001f,
 * Triangulation.cpp:24-60).  28 bytes. */
typedef struct mage_stereo_point {
    int32_t query_idx, train_idx; /* frame 0's keypoint, frame 1's keypoint */
    float distance;
    float position[3];
    uint32_t near_parallel;
} mage_stereo_point;

/* Verdict of a match: TriangulatePoints' first reason to drop it, in its order. */
#define MAGE_ST_ACCEPTED 0
#define MAGE_ST_EPIPOLAR 1       /* both epipolar distances sum over 2 * MaxEpipolarError (:945-950) */
#define MAGE_ST_BEHIND 2         /* VerifyProjectInFront of frame 0, then frame 1 (:956-960) */
#define MAGE_ST_DISTANCE_RATIO 3 /* |X - C0| / |C0 - C1| < MinAcceptedDistanceRatio (:966-974) */
#define MAGE_ST_OCTAVE 4         /* the two keypoints' octaves differ (:977-980) */
#define MAGE_ST_BAD_INDEX 5      /* queryIdx / trainIdx is not a keypoint: nothing read */

/* Bits of a pair's status word. */
#define MAGE_ST_STATUS_OVER_LIMIT 1u /* a frame has more than 4096 keypoints, or more than its pitch */
#define MAGE_ST_STATUS_OVER_CAP 2u   /* more accepted matches than `cap` (the count reports cap) */

/* Initialize's device stage for `pairs` stereo pairs, three launches on `stream` with no host step
 * between them:
 *   a. CreateFilteredDescriptorMask(-1, crop, frame0) (StereoMapInit.cpp:28-45, :104-105): frame
 *      0's mask byte per keypoint from IsWithinArea(kp.pt, crop) (Utils/cv.h:421-427: x in
 *      [crop.x, crop.x + width), y in [crop.y, crop.y + height] — the bottom edge is inside), the
 *      true count in d_n_masked[pair]; frame 1 is unmasked (:107-108).  The masked descriptors are
 *      packed in keypoint order, as Match packs descriptorMatrixA (FeatureMatcher.cpp:84-108).
 *   b. Match (:112) by mage_hamming_match_batch_device over the packed frame 0 (A) and frame 1 (B)
 *      with the settings' MaxHammingDistance / MinHammingDifference; queryIdx is mapped back to
 *      frame 0's keypoint index, so d_matches / d_n_matches hold Match's result (ascending
 *      queryIdx; a count over match_cap means only match_cap were kept).
 *   c. MapInitialization::TriangulatePoints (Tracking/MapInitialization.cpp:911-986) over the
 *      matches in order, frame 0 the reference frame and frame 1 the current frame:
 *      d_verdict[pair * match_cap + m] = MAGE_ST_*; the accepted matches in match order at
 *      d_out + pair * cap, their count (at most cap) in d_n_out[pair]; and the bundle adjustment's
 *      inputs as BundleAdjustInitializationData enumerates them (:1099-1110, frame-major) for the
 *      n = d_n_out[pair] points: d_ba_points + pair * 3 cap (n x 3), and 2n observations at
 *      pair * 2 cap of d_ba_uv (2 floats each), d_ba_cam, d_ba_pt and d_ba_info — observation i
 *      is point i in frame 0 (cam 0, frame 0's keypoint position), observation n + i point i in
 *      frame 1; info = MapPointRefinementConfidence(1) (init points are created with refinement
 *      count 1, StereoMapInit.cpp:77).  These are mage_ba_set_points / mage_ba_set_observations'
 *      arguments.
 * Per pair: poses as mage_ba_set_cameras takes them, frame 0 then frame 1 (d_pos3 6 floats, d_r9
 * 18, d_intr4 8 = {cx, cy, fx, fy} twice); d_crop the cv::Rect {x, y, width, height} of
 * CalculateOverlapCropSourceInTarget (:100); frame f's keypoints and 32-byte descriptors pitch0 /
 * pitch1 entries per pair, counts d_n0 / d_n1.  d_mask0: pitch0 bytes per pair.  d_scratch: pairs
 * x pitch0 x 36 bytes, 16-byte aligned like the descriptors.
 * d_desc0 == NULL skips (b): d_matches / d_n_matches are then inputs (queryIdx = frame 0's
 * keypoint), read as above, and d_desc1 / d_scratch are not used.
 * d_status[pair] is written (not ORed): MAGE_ST_STATUS_OVER_LIMIT for a pair with a keypoint count
 * over 4096 or over its pitch — that pair reports 0 masked keypoints, 0 matches from (b) and 0
 * points, and its mask and verdict bytes are left untouched; MAGE_ST_STATUS_OVER_CAP when more
 * matches were accepted than cap.  Nothing is written past a pair's counts: mask bytes past
 * d_n0[pair], verdicts past min(d_n_matches[pair], match_cap), records and points past
 * d_n_out[pair], observations past 2 d_n_out[pair].  The other pairs are unaffected. */
mage_status mage_stereo_init_triangulate_batch_device(
    const mage_stereo_init_settings* settings, uint32_t pairs, const float* d_pos3, const float* d_r9,
    const float* d_intr4, const int32_t* d_crop, const mage_keypoint* d_kp0, const uint8_t* d_desc0, int64_t pitch0,
    const uint32_t* d_n0, const mage_keypoint* d_kp1, const uint8_t* d_desc1, int64_t pitch1, const uint32_t* d_n1,
    uint8_t* d_mask0, uint32_t* d_n_masked, mage_dmatch* d_matches, uint32_t match_cap, uint32_t* d_n_matches,
    uint8_t* d_verdict, mage_stereo_point* d_out, uint32_t cap, uint32_t* d_n_out, float* d_ba_points, float* d_ba_uv,
    uint32_t* d_ba_cam, uint32_t* d_ba_pt, float* d_ba_info, uint32_t* d_status, void* d_scratch, mage_stream stream);

/* One pair, host buffers, synchronous, runs on `device`: arrays as one pair of the batched form.
 * With desc0 / desc1 (n x 32 bytes) the matcher runs and `matches` (match_cap records, at least
 * one) and *n_matches are outputs — Match's result, queryIdx = frame 0's keypoint; a result
 * longer than match_cap is cut to its first match_cap.  With desc0 == NULL the first *n_matches
 * records of `matches` are the input.  verdict: one byte per match; out and ba_* sized for cap
 * points (cap == 0: every accepted match is over the capacity).  More than 4096 keypoints in a
 * frame sets MAGE_ST_STATUS_OVER_LIMIT in *status and writes nothing else. */
mage_status mage_stereo_init_triangulate(const mage_stereo_init_settings* settings, const float* pos3, const float* r9,
                                         const float* intr4, const int32_t crop_xywh[4], const mage_keypoint* kp0,
                                         const uint8_t* desc0, uint32_t n0, const mage_keypoint* kp1,
                                         const uint8_t* desc1, uint32_t n1, mage_dmatch* matches, uint32_t match_cap,
                                         uint32_t* n_matches, uint8_t* mask0, uint32_t* n_masked, uint8_t* verdict,
                                         mage_stereo_point* out, uint32_t cap, uint32_t* n_out, float* ba_points,
                                         float* ba_uv, uint32_t* ba_cam, uint32_t* ba_pt, float* ba_info,
                                         uint32_t* status, int device);

/* Stages (a) and (c) for one pair in plain C++ on the calling thread, the matches given (queryIdx
 * = frame 0's keypoint): the reference's sequential loops over the same per-match arithmetic, the
 * CPU backend, bit-identical to the kernels.  Arrays as one pair of the batched form, ba_* sized
 * for cap points.  No GPU. */
mage_status mage_stereo_init_triangulate_host(const mage_stereo_init_settings* settings, const float* pos3,
                                              const float* r9, const float* intr4, const int32_t crop_xywh[4],
                                              const mage_keypoint* kp0, uint32_t n0, const mage_keypoint* kp1,
                                              uint32_t n1, const mage_dmatch* matches, uint32_t n_matches,
                                              uint8_t* mask0, uint32_t* n_masked, uint8_t* verdict,
                                              mage_stereo_point* out, uint32_t cap, uint32_t* n_out, float* ba_points,
                                              float* ba_uv, uint32_t* ba_cam, uint32_t* ba_pt, float* ba_info,
                                              uint32_t* status);

/* What StereoMapInit::Initialize returns: boost::none for four reasons, or the InitializationData. */
#define MAGE_STEREO_INIT_OK 0
#define MAGE_STEREO_INIT_ZERO_DISPLACEMENT 1 /* |translation of frame0ToFrame1| < 0.00001 (:139) */
#define MAGE_STEREO_INIT_FEW_MATCHES 2       /* fewer than MinFeatureMatches matches (:151) */
#define MAGE_STEREO_INIT_FEW_POINTS 3        /* fewer than MinInitMapPoints accepted matches (:161) */
#define MAGE_STEREO_INIT_FAILED_VALIDATION 4 /* ValidateInitializationData (:183) */

typedef struct mage_stereo_map_init_result {
    int32_t code;          /* MAGE_STEREO_INIT_* */
    int32_t crop[4];       /* frame0CropRect {x, y, width, height} (:100) */
    uint32_t n_masked;     /* numFilteredDescriptorsFrame0 (:105) */
    uint32_t n_matches;    /* numMatches (:112) */
    uint32_t n_verdicts;   /* n_matches once TriangulatePoints ran (code >= FEW_POINTS or OK), else 0 */
    float frame1_pos3[3];  /* frame 1's pose, view-space t and column-major R as mage_ba_set_cameras */
    float frame1_r9[9];    /*   takes them: after the bundle adjustment, else as normalised, else identity */
    uint32_t n_points;     /* surviving map points */
    uint32_t n_ba_outliers;
    uint32_t ba_runs;      /* StepBundleAdjustment calls (RunBundleAdjustment's return value) */
} mage_stereo_map_init_result;

/* StereoMapInit::Initialize (Stereo/StereoMapInit.cpp:97-194) for one pair of analysed frames, host
 * buffers, synchronous, on `device`, in the reference's order:
 *   1. the crop (:100, mage_overlap_crop_source_in_target with MaxDepthMeters), frame 0's mask and the
 *      two-way Match (:104-114) — on the GPU, with step 4 behind them in the same chain;
 *   2. frame0ToFrame1's translation normalised to length 1, in float (:135-148); a length below
 *      0.00001 is ZERO_DISPLACEMENT (reported even when there are too few matches as well);
 *   3. fewer than MinFeatureMatches matches is FEW_MATCHES;
 *   4. InitializeWithFrames (:47-88): frame 0 at the identity, frame 1 at Pose{normalized.inv()} — the
 *      LU inverse is the pose's inverse view matrix and its view matrix is Invert() of that
 *      (Data/Pose.cpp:31-36) — and TriangulatePoints over the matches;
 *   5. fewer than MinInitMapPoints accepted matches is FEW_POINTS;
 *   6. AddExtrinsicTether(frame 0, InitializationTetherStrength) (:168, KeyframeBuilder.h:38-48) and
 *      BundleAdjustInitializationData (MapInitialization.cpp:1096-1226): camera 0 fixed, points free,
 *      RunBundleAdjustment's schedule with the NoOpScheduler (BundleAdjust.cpp:293-346: runs of
 *      NumStepsPerRun steps at HuberWidth, the outlier bound starting at BundleAdjustSettings.
 *      MaxOutlierError and multiplied by MaxOutlierErrorScaleFactor^2 after every run, until NumSteps
 *      steps or a residual <= MinMeanSquareError after MinSteps), the tether through
 *      mage_ba_set_tethers(MAGE_TETHER_TRANSFORM) after BuildDataForG2O's second inversion
 *      (BundleAdjust.cpp:177-192); frame 1's pose from GetPose, the points from GetPoint; every
 *      outlier association removed and every point left with fewer than 2 removed by swap-with-back
 *      (:1166-1222);
 *   7. ValidateInitializationData (:1228-1268): the point count, |normalised world z| of frame 1 over
 *      MaxPoseContributionZ, its distance from the origin outside [1 / AmountBACanChangePose,
 *      AmountBACanChangePose] -> FAILED_VALIDATION.
 * A failure is a normal return (MAGE_OK with the code set).  The cameras are frame 0's and frame 1's
 * undistorted calibrations and sizes (extrinsics not read).  Outputs, each with room for n0 entries
 * (ba_outliers: 2 n0 per bundle adjustment run): mask0 and matches[0 .. n_matches) always; verdict[0
 * .. n_verdicts) from step 4 on; points[0 .. n_points) — the surviving points in the reference's
 * order after its swaps, position from the bundle adjustment, query_idx / train_idx the two
 * keyframes' associations — and ba_outliers[0 .. n_ba_outliers), observation indices over the runs
 * (observation o < n is accepted match o in frame 0, o >= n match o - n in frame 1), from step 6
 * on.  More than 4096 keypoints in a frame is MAGE_EUNSUPPORTED. */
mage_status mage_stereo_map_init(const mage_stereo_init_settings* settings, const float frame0_to_frame1[16],
                                 const mage_camera_config* camera0, const mage_camera_config* camera1,
                                 const mage_keypoint* kp0, const uint8_t* desc0, uint32_t n0, const mage_keypoint* kp1,
                                 const uint8_t* desc1, uint32_t n1, mage_stereo_map_init_result* result, uint8_t* mask0,
                                 mage_dmatch* matches, uint8_t* verdict, mage_stereo_point* points,
                                 uint32_t* ba_outliers, int device);

/* Debug view of mage_stereo_map_init's host arithmetic, no device; each part runs when its first
 * pointer is given.  frame0_to_frame1: step 2 and 4's scalars (the zero-displacement flag, the
 * normalised matrix, frame 1's pose) and the 7 tether parameters of step 6.  order: the culling of
 * step 6 for n_points accepted matches and the given outlier observation indices -> the surviving
 * points' indices in output order, *n_left of them.  valid: step 7 for frame 1's pose ba_pos3 /
 * ba_r9 and the surviving count (n_points when `order` is not given). */
mage_status mage_debug_stereo_init_host(const mage_stereo_init_settings* settings, const float frame0_to_frame1[16],
                                        int32_t* zero_displacement, float normalized[16], float pos3[3], float r9[9],
                                        float tether7[7], uint32_t n_points, const uint32_t* outliers,
                                        uint32_t n_outliers, uint32_t* order, uint32_t* n_left, const float* ba_pos3,
                                        const float* ba_r9, int32_t* valid);

/* ------------------------------------------------------------------------------------------ */
/* Monocular map initialisation — the two-view geometry of                                     */
/* MapInitialization::InitializeWithFrames (Core/.../Tracking/MapInitialization.cpp:988-1094)  */
/* ------------------------------------------------------------------------------------------ */

/* MonoMapInitializationSettings (MageSettings.h:95-128) in the reference's order: its scalars, then
 * its two OrbMatcherSettings bags (FivePointMatchingSettings, ExtraFrameMatchingSettings).
 * struct_size must be sizeof(mage_mono_init_settings); anything else is MAGE_EINVAL.  The two-view
 * stage reads the fields marked (*), the third-frame stage (mage_mono_init_third_frame*) those
 * marked (3); the others belong to the rest of TryIntializeMapWithProvidedFrames (new points, the
 * bundle adjustments, validation) and are carried for it. */
typedef struct mage_mono_init_settings {
    uint32_t struct_size;
    float fundamental_transfer_error_threshold;  /* (*) FundamentalTransferErrorThreshold 1.1 */
    uint32_t min_feature_matches;                /* (*) MinFeatureMatches 65, at least 5 */
    uint32_t min_scoring_inliers;                /* (*) MinScoringInliers 50 */
    float min_inlier_percentage;                 /* (*) MinInlierPercentage 0.5 */
    uint32_t min_initial_map_points;             /* MinInitialMapPoints 40 */
    uint32_t min_map_points;                     /* MinMapPoints 60 */
    float min_third_frame_match_percentage;      /* (3) MinThirdFrameMatchPercentage 0.5 */
    float feature_covisibility_threshold;        /* FeatureCovisibilityThreshold 0.35 */
    float max_parallax_3d_distance;              /* (*) MaxParallax3dDistance 500 */
    float max_parallax_3d_median_distance;       /* (*) MaxParallax3dMedianDistance 20 */
    float min_candidate_pose_disimilarity;       /* (*) MinCandidatePoseDisimilarity 0.3 */
    float max_pose_contribution_z;               /* (*) MaxPoseContributionZ 0.66 */
    uint32_t bundle_adjustment_g2o_steps;        /* BundleAdjustmentG2OSteps 5 */
    float bundle_adjustment_huber_width;         /* BundleAdjustmentHuberWidth 1.5 */
    uint32_t ransac_iterations_for_models;       /* (*) RansacIterationsForModels 90, in 1..256 */
    float max_epipolar_error;                    /* (*) MaxEpipolarError 3.5 */
    float max_outlier_error;                     /* MaxOutlierError 2.5 */
    float amount_ba_can_change_pose;             /* AmountBACanChangePose 1.65 */
    float map_initialization_new_points_creation_min_distance; /* ...NewPointsCreationMinDistance 0.25 */
    uint32_t map_init_frame_interval_milliseconds;       /* MapInitFrameIntervalMilliseconds 0 */
    uint32_t min_initialization_interval_milliseconds;   /* MinInitializationIntervalMilliseconds 150 */
    uint32_t max_initialization_interval_milliseconds;   /* MaxInitializationIntervalMilliseconds 540 */
    float min_pixel_spread;                      /* (*) MinPixelSpread 40 */
    float final_ba_huber_width;                  /* FinalBA_HuberWidth 0.9 */
    float final_ba_max_outlier_error;            /* FinalBA_MaxOutlierError 4 */
    float final_ba_max_outlier_error_scale_factor; /* FinalBA_MaxOutlierErrorScaleFactor 0.75 */
    float final_ba_min_mean_square_error;        /* FinalBA_MinMeanSquareError 0 */
    uint32_t final_ba_num_steps_per_run;         /* FinalBA_NumStepsPerRun 5 */
    uint32_t final_ba_num_steps;                 /* FinalBA_NumSteps 15 */
    float extra_frame_max_outlier_error;         /* (3) ExtraFrame_MaxOutlierError 8 */
    uint32_t extra_frame_bundle_adjustment_steps; /* (3) ExtraFrame_BundleAdjustmentSteps 5 */
    float extra_frame_huber_width;               /* (3) ExtraFrame_HuberWidth 4 */
    float extra_frame_search_radius;             /* (3) ExtraFrame_SearchRadius 40 */
    int32_t five_point_max_hamming_distance;     /* (*) (3) FivePointMatchingSettings.MaxHammingDistance 30 */
    int32_t five_point_min_hamming_difference;   /* (*) (3) FivePointMatchingSettings.MinHammingDifference 1 */
    int32_t extra_frame_max_hamming_distance;    /* (3) ExtraFrameMatchingSettings.MaxHammingDistance 30 */
    int32_t extra_frame_min_hamming_difference;  /* (3) ExtraFrameMatchingSettings.MinHammingDifference 1 */
} mage_mono_init_settings;

/* A pair's verdict: InitializeWithFrames' reasons to give up, in its order. */
#define MAGE_MI_OK 0
#define MAGE_MI_FEW_MATCHES 1   /* fewer than MinFeatureMatches matches (:592, :1002) */
#define MAGE_MI_NO_HYPOTHESIS 2 /* FindPossiblePoses returned nothing (:1014-1019) */
#define MAGE_MI_NO_VALID_POSE 3 /* FindCorrectPose: no pose with a valid score (:453) */
#define MAGE_MI_TOO_SIMILAR 4   /* the best two poses' scores are too similar (:460-465) */
#define MAGE_MI_Z_BIASED 5      /* the best pose moves too much along Z (:468-472) */

/* Bits of a pair's status word. */
#define MAGE_MI_STATUS_OVER_LIMIT 1u /* over 4096 keypoints in a frame or over its pitch, over 4096 matches or over match_cap */
#define MAGE_MI_STATUS_OVER_CAP 2u   /* more accepted matches than `cap` (the count reports cap) */
#define MAGE_MI_STATUS_BAD_INDEX 4u  /* a given match names no keypoint */

/* Bits of mage_mono_init_result.cand_flags. */
#define MAGE_MI_POSE_TWISTED 1u   /* skipped: its right vector opposes the reference's (:362) */
#define MAGE_MI_POSE_ENOUGH 2u    /* passed the MinScoringInliers / MinInlierPercentage gate (:419) */
#define MAGE_MI_POSE_MEDIAN_OK 4u /* its median depth is within MaxParallax3dMedianDistance (:433) */

/* What the two-view stage decides for one pair; written whole for every pair, zero where a stage
 * was not reached.  Poses are as mage_ba_set_cameras takes them: view-space t and column-major R. */
typedef struct mage_mono_init_result {
    uint32_t verdict;    /* MAGE_MI_* */
    uint32_t status;     /* MAGE_MI_STATUS_* bits; with OVER_LIMIT or BAD_INDEX nothing else of the pair is written */
    uint32_t n_matches;  /* the matches the stage ran on */
    uint32_t n_points;   /* accepted records (at most cap); 0 unless the verdict is MAGE_MI_OK */
    int32_t win_iteration, win_root; /* FindPossiblePoses' winner: RANSAC iteration and root, or -1 */
    int32_t win_indices[5];          /* its five matches, ascending */
    float win_score;                 /* its ScoreFundamentalMatrix */
    int32_t selected_pose;           /* FindCorrectPose's selectedPoseIndex, or -1 */
    float next_best_score;           /* its nextBestPoseScore */
    float pos3[6], r9[18];           /* frame 0 (the identity) and frame 1 (the selected pose when OK, else the identity) */
    float cand_pos3[12], cand_r9[36]; /* FindEssentialPotientialPoses' four poses of the winner, in its order */
    float cand_score[4];             /* FindCorrectPose's score per pose */
    float cand_median[4];            /* its median depth (0 unless MAGE_MI_POSE_ENOUGH) */
    uint32_t cand_count[4];          /* its candidatePosePoints.size() */
    uint32_t cand_flags[4];          /* MAGE_MI_POSE_* */
} mage_mono_init_result;

/* Bytes of one pair's trace for `iterations` RANSAC iterations, arrays in this order:
 *   int32 indices[iterations][5]    the sample's matches, ascending, or -1 five times (no sample);
 *   int32 candidates[iterations]    essential matrices the five-point solver returned (0..10);
 *   float E[iterations][10][9]      they, row-major, in root order; zero past the count;
 *   float score[iterations][10]     ScoreFundamentalMatrix (0 when gated out or past the count);
 *   uint32 inliers[iterations][10]  its inlier count;
 *   uint32 cheirality[iterations][10]  1 when HasConsistentCheirality on the sample's points.
 * 504 bytes per iteration. */
uint64_t mage_mono_init_trace_bytes(uint32_t iterations);

/* Bytes of mage_mono_init_two_view_batch_device's scratch: the work buffer (pairs traces, when no
 * trace is given) and, with the matcher, the packed octave-0 descriptors of both frames with their
 * keypoint indices and counts. */
uint64_t mage_mono_init_scratch_bytes(uint32_t iterations, uint32_t pairs, int64_t pitch0, int64_t pitch1,
                                      int32_t with_trace, int32_t with_matcher);

/* The two-view stage for `pairs` frame pairs, launches on `stream` with no host step between them:
 *   m. (with descriptors) the octave-0 masks of :562-583 for both frames, their descriptors packed
 *      in keypoint order, Match (:585) by mage_hamming_match_batch_device with
 *      FivePointMatchingSettings, and the indices mapped back to keypoints: d_matches /
 *      d_n_matches then hold Match's result.  With d_desc0 == NULL they are inputs — the caller's
 *      bestMatches after its covisibility counters (:611-623), which stay caller-side.
 *   a. CollectMatchPoints (:889-909) and FindPossiblePoses' sampler (:196-249).
 *   b. the five-point solver per hypothesis (Tracking/ComputeEssential.cpp:357-514).
 *   c. ScoreFundamentalMatrix (:279-322) and HasConsistentCheirality (:129-179) per candidate.
 *   d. the winner (the earliest maximum score among the consistent candidates), its four poses
 *      (:85-114), FindCorrectPose (:324-480), and for MAGE_MI_OK the accepted matches of the selected
 *      pose compacted in match order at d_out + pair * cap with the bundle adjustment's inputs laid
 *      out as mage_stereo_init_triangulate_batch_device lays them out (frame-major, info =
 *      MapPointRefinementConfidence(1)).
 * Per pair: d_intr4 8 floats = {cx, cy, fx, fy} of frame 0 then frame 1; frame f's keypoints and
 * 32-byte descriptors pitch0 / pitch1 entries per pair, counts d_n0 / d_n1; d_matches match_cap
 * records per pair.  d_trace: NULL, or pairs x mage_mono_init_trace_bytes(iterations) bytes.
 * d_scratch: mage_mono_init_scratch_bytes(...) bytes, 16-byte aligned like the descriptors; may be
 * NULL when that is 0.  Nothing is written past a pair's counts: records and points past
 * n_points, observations past 2 n_points; the trace of a pair that stops before (a) (over a limit,
 * a bad index, too few matches) is left untouched.  The other pairs are unaffected. */
mage_status mage_mono_init_two_view_batch_device(
    const mage_mono_init_settings* settings, uint32_t pairs, const float* d_intr4, const mage_keypoint* d_kp0,
    const uint8_t* d_desc0, int64_t pitch0, const uint32_t* d_n0, const mage_keypoint* d_kp1, const uint8_t* d_desc1,
    int64_t pitch1, const uint32_t* d_n1, mage_dmatch* d_matches, uint32_t match_cap, uint32_t* d_n_matches,
    mage_mono_init_result* d_result, mage_stereo_point* d_out, uint32_t cap, float* d_ba_points, float* d_ba_uv,
    uint32_t* d_ba_cam, uint32_t* d_ba_pt, float* d_ba_info, void* d_trace, void* d_scratch, mage_stream stream);

/* One pair, host buffers, synchronous, runs on `device`: arrays as one pair of the batched form.
 * With desc0 / desc1 (n x 32 bytes) the matcher runs and `matches` (match_cap records, at least
 * one) and *n_matches are outputs; with desc0 == NULL the first *n_matches records are the input.
 * out and ba_* sized for cap points; trace NULL or mage_mono_init_trace_bytes(iterations) bytes. */
mage_status mage_mono_init_two_view(const mage_mono_init_settings* settings, const float* intr4,
                                    const mage_keypoint* kp0, const uint8_t* desc0, uint32_t n0,
                                    const mage_keypoint* kp1, const uint8_t* desc1, uint32_t n1, mage_dmatch* matches,
                                    uint32_t match_cap, uint32_t* n_matches, mage_mono_init_result* result,
                                    mage_stereo_point* out, uint32_t cap, float* ba_points, float* ba_uv,
                                    uint32_t* ba_cam, uint32_t* ba_pt, float* ba_info, void* trace, int device);

/* Stages (a) to (d) for one pair in plain C++ on the calling thread, the matches given: the
 * reference's sequential loops over the same arithmetic, the CPU backend, bit-identical to the
 * kernels.  No GPU. */
mage_status mage_mono_init_two_view_host(const mage_mono_init_settings* settings, const float* intr4,
                                         const mage_keypoint* kp0, uint32_t n0, const mage_keypoint* kp1, uint32_t n1,
                                         const mage_dmatch* matches, uint32_t n_matches,
                                         mage_mono_init_result* result, mage_stereo_point* out, uint32_t cap,
                                         float* ba_points, float* ba_uv, uint32_t* ba_cam, uint32_t* ba_pt,
                                         float* ba_info, void* trace);

/* The third frame of TryIntializeMapWithProvidedFrames (MapInitialization.cpp:695-840): the middle
 * frame is placed half way between the initialisation pair, every map point is looked up in it
 * twice (frame 0's descriptor under ExtraFrameMatchingSettings, frame 1's under
 * FivePointMatchingSettings) against one shared mask of unassociated keypoints, the better match
 * takes the keypoint, a pose-only bundle adjustment culls outliers, and two gates on
 * MinThirdFrameMatchPercentage decide. */

/* A problem's verdict. */
#define MAGE_M3_OK 0
#define MAGE_M3_FEW_MATCHES 1    /* too few associations after the matching (:803), or no map points */
#define MAGE_M3_FEW_AFTER_CULL 2 /* too few left after the outliers were culled (:835) */

/* Bits of a problem's status word. */
#define MAGE_M3_STATUS_OVER_LIMIT 1u /* over 4096 points or third-frame keypoints, or a count over its pitch / cap */
#define MAGE_M3_STATUS_BAD_INDEX 2u  /* a point's keypoint index names no keypoint of frame 0 / frame 1 */

/* A point's verdict byte. */
#define MAGE_M3_PT_BEHIND 0   /* projected behind the midpoint camera (:728): never searched */
#define MAGE_M3_PT_NO_MATCH 1 /* neither query matched */
#define MAGE_M3_PT_FRAME0 2   /* took the match of frame 0's descriptor */
#define MAGE_M3_PT_FRAME1 3   /* took the match of frame 1's descriptor (strictly closer, or the only one) */
#define MAGE_M3_PT_CULLED 4   /* matched, then culled as an outlier of the pose bundle adjustment (:829-832) */

/* Written whole for every problem; with a status bit set the rest is zero apart from n_points and
 * nothing else of the problem is written.  Poses as mage_ba_set_cameras takes them.  The reference
 * keeps the MIDPOINT pose for the frame (:840) and drops the optimised one; both are reported. */
typedef struct mage_mono_init_third_result {
    uint32_t verdict;      /* MAGE_M3_* */
    uint32_t status;       /* MAGE_M3_STATUS_* bits */
    uint32_t n_points;     /* the map points given */
    uint32_t n_behind;     /* skipped: Distance < 0 */
    uint32_t n_matched;    /* associations after the matching */
    uint32_t n_outliers;   /* culled by the bundle adjustment (0 when it did not run) */
    uint32_t n_associated; /* n_matched - n_outliers: the observations written */
    float mean_sq;         /* the bundle adjustment's mean square error (0 when it did not run) */
    float pos3[3], r9[9];         /* the frame's pose: the midpoint pose */
    float opt_pos3[3], opt_r9[9]; /* OptimizeCameraPose's result (zero when it did not run) */
} mage_mono_init_third_result;

/* Bytes of mage_mono_init_third_frame_batch_device's scratch.  offsets: NULL, or 13 words that
 * receive the byte offsets of its arrays, in this order: obs_start (problems + 1 uint32, the prefix
 * of ba_count), ba_count (per problem the observations handed to the bundle adjustment: n_matched,
 * or 0 after a failed first gate), ba_pos3, ba_r9 (its start, the midpoint pose), matched
 * (problems x cap uint32: the matched points' indices in point order), ba_points (3 floats), ba_uv
 * (2 floats), ba_info, outlier (uint8) per observation, prefix-packed over the problems, and the
 * bundle adjustment's opt_pos3, opt_r9, mean_sq and opt_qt7 (its fp64 state, 7 doubles) per problem. */
uint64_t mage_mono_init_third_scratch_bytes(uint32_t problems, uint32_t cap, uint64_t* offsets);

/* `problems` independent third frames, launches on `stream` with no host step between them: the
 * match kernel (midpoint pose, projection, both queries per point in order, the first gate), a
 * scan-and-pack launch, mage_ba_pose_batch_device (ExtraFrame_BundleAdjustmentSteps x
 * ExtraFrame_HuberWidth, ExtraFrame_MaxOutlierError^2, info = MapPointRefinementConfidence(1)) and
 * the finish kernel (cull, second gate, compaction).
 * Per problem: d_intr4 4 floats {cx, cy, fx, fy} of the third frame; d_pos3 6 / d_r9 18 floats, the
 * poses of frame 0 then frame 1; d_points cap x 3 floats with d_n_points[p] of them used, in
 * initializationData.MapPoints order; d_idx0 / d_idx1 cap words, each point's keypoint in frame 0 /
 * frame 1; d_desc0 / d_desc1 the two frames' 32-byte descriptors, pitch0 / pitch1 per problem, counts
 * d_n0 / d_n1; the third frame's keypoints and descriptors pitch2 per problem, count d_n2 (only its
 * octave-0 keypoints are candidates: the query octave is 0).  Descriptor pointers 16-byte aligned.
 * Outputs per problem: d_result; cap words d_keypoint (the point's keypoint in the third frame, -1
 * when it has none or lost it), cap bytes d_verdict (MAGE_M3_PT_*), 2 x cap words d_dist (the best
 * distance of query 0 and of query 1 among the candidates the point saw at its turn, -1 when there
 * was none), 2 x cap floats d_proj (every point's ProjectUndistorted position, behind or not); pitch2
 * bytes d_mask (1 = still unassociated after the matching; taken keypoints stay
 * taken when their point is culled, as in the reference); and the surviving associations compacted in
 * point order as bundle-adjustment observations, n_associated of them: d_obs_uv (2 floats), d_obs_pt
 * (the point's index), d_obs_cam (cam_index), d_obs_info.  Nothing is written past a problem's
 * counts.  d_scratch: mage_mono_init_third_scratch_bytes(problems, cap, NULL) bytes, 256-byte
 * aligned. */
mage_status mage_mono_init_third_frame_batch_device(
    const mage_mono_init_settings* settings, uint32_t problems, const float* d_intr4, const float* d_pos3,
    const float* d_r9, const float* d_points, uint32_t cap, const uint32_t* d_n_points, const int32_t* d_idx0,
    const int32_t* d_idx1, const uint8_t* d_desc0, int64_t pitch0, const uint32_t* d_n0, const uint8_t* d_desc1,
    int64_t pitch1, const uint32_t* d_n1, const mage_keypoint* d_kp2, const uint8_t* d_desc2, int64_t pitch2,
    const uint32_t* d_n2, uint32_t cam_index, mage_mono_init_third_result* d_result, int32_t* d_keypoint,
    uint8_t* d_verdict, int32_t* d_dist, float* d_proj, uint8_t* d_mask, float* d_obs_uv, uint32_t* d_obs_pt, uint32_t* d_obs_cam,
    float* d_obs_info, void* d_scratch, mage_stream stream);

/* One problem, host buffers, synchronous, runs on `device`: arrays as one problem of the batched
 * form with cap = n_points and the pitches equal to the counts.  outlier: NULL, or n_points bytes
 * that receive the bundle adjustment's flag per matched point, in point order (n_matched of them;
 * none after a failed first gate). */
mage_status mage_mono_init_third_frame(const mage_mono_init_settings* settings, const float* intr4, const float* pos3,
                                       const float* r9, const float* points, uint32_t n_points, const int32_t* idx0,
                                       const int32_t* idx1, const uint8_t* desc0, uint32_t n0, const uint8_t* desc1,
                                       uint32_t n1, const mage_keypoint* kp2, const uint8_t* desc2, uint32_t n2,
                                       uint32_t cam_index, mage_mono_init_third_result* result, int32_t* keypoint,
                                       uint8_t* verdict, int32_t* dist, float* proj, uint8_t* mask, float* obs_uv,
                                       uint32_t* obs_pt, uint32_t* obs_cam, float* obs_info, uint8_t* outlier,
                                       int device);

/* The same in plain C++ on the calling thread: the reference's sequential loop, literally, the CPU
 * backend; its matching half is bit-identical to the match kernel.  The library has no host pose
 * bundle adjustment, so its outcome is an input: outlier NULL stops after the first gate (the record
 * as the match kernel leaves it, no observations written); otherwise n_matched flags in point order
 * with the optimised pose opt_pos3 / opt_r9 and mean_sq, and the cull, the second gate and the
 * compaction run (ignored after a failed first gate, where the observations are all the matches).
 * ba_points / ba_uv / ba_info: NULL, or n_points x 3 / 2 / 1 floats that receive the bundle
 * adjustment's inputs, n_matched of them.  No GPU. */
mage_status mage_mono_init_third_frame_host(const mage_mono_init_settings* settings, const float* intr4,
                                            const float* pos3, const float* r9, const float* points,
                                            uint32_t n_points, const int32_t* idx0, const int32_t* idx1,
                                            const uint8_t* desc0, uint32_t n0, const uint8_t* desc1, uint32_t n1,
                                            const mage_keypoint* kp2, const uint8_t* desc2, uint32_t n2,
                                            uint32_t cam_index, const uint8_t* outlier, const float* opt_pos3,
                                            const float* opt_r9, float mean_sq, mage_mono_init_third_result* result,
                                            int32_t* keypoint, uint8_t* verdict, int32_t* dist, float* proj,
                                            uint8_t* mask, float* obs_uv, uint32_t* obs_pt, uint32_t* obs_cam,
                                            float* obs_info, float* ba_points, float* ba_uv, float* ba_info);

/* ------------------------------------------------------------------------------------------ */
/* Relocalisation — PoseEstimator::PNPRansac (Core/.../Tracking/PoseEstimator.cpp:610-638) as   */
/* TryEstimatePoseFromCandidates uses it (:219-437): a pose from 2D-3D matches with no prior   */
/* ------------------------------------------------------------------------------------------ */

/* RelocalizationSettings (MageSettings.h:236-250) in the reference's order, then its
 * OrbMatcherSettings bag.  struct_size must be sizeof(mage_reloc_settings); anything else is
 * MAGE_EINVAL.  The PnP stage reads the fields marked (*); the others belong to the rest of
 * TryEstimatePoseFromCandidates (the bundle adjustments, the guided search) and are carried for it. */
typedef struct mage_reloc_settings {
    uint32_t struct_size;
    uint32_t min_brute_force_correspondences;   /* (*) MinBruteForceCorrespondences 20 */
    uint32_t min_radius_match_correspondences;  /* MinRadiusMatchCorrespondences 15 */
    uint32_t min_map_points;                    /* MinMapPoints 10 */
    float ransac_inliers_pct_required;          /* (*) RansacInliersPctRequired 0.4 */
    float bundle_adjust_inliers_pct_required;   /* BundleAdjustInliersPctRequired 0.4 */
    float ransac_confidence;                    /* (*) RansacConfidence 0.6, in (0, 1) exclusive */
    uint32_t round_robin_iterations;            /* RoundRobinIterations 5 */
    uint32_t ransac_iterations;                 /* (*) RansacIterations 2, in 1..256 */
    uint32_t bundle_adjust_iterations;          /* BundleAdjustIterations 10 */
    float search_radius;                        /* SearchRadius 20 */
    float max_bundle_adjust_reprojection_error; /* MaxBundleAdjustReprojectionError 8 */
    float max_bundle_pnp_reprojection_error;    /* (*) MaxBundlePnPReprojectionError 8 */
    int32_t max_hamming_distance;               /* OrbMatcherSettings.MaxHammingDistance 30 */
    int32_t min_hamming_difference;             /* OrbMatcherSettings.MinHammingDifference 1 */
} mage_reloc_settings;

/* A problem's verdict. */
#define MAGE_RP_OK 0
#define MAGE_RP_FEW_MATCHES 1 /* fewer than MinBruteForceCorrespondences matches (:291) */
#define MAGE_RP_NO_MODEL 2    /* PNPRansac returned false (:319-324): under five matches, or no hypothesis with five inliers */
#define MAGE_RP_FEW_INLIERS 3 /* inFront / matches < RansacInliersPctRequired (:339); the candidate stays worthwhile */

/* Bits of a problem's status word. */
#define MAGE_RP_STATUS_OVER_LIMIT 1u /* over 4096 matches or over match_cap, or more keypoints than kp_pitch */
#define MAGE_RP_STATUS_OVER_CAP 2u   /* more kept inliers than `cap` (n_kept reports cap) */
#define MAGE_RP_STATUS_BAD_INDEX 4u  /* a match names no keypoint, or a candidate keypoint with no map point */

/* What the stage decides for one problem; written whole for every problem, zero (indices -1, the
 * pose the identity) where a step was not reached.  The pose is as mage_ba_pose_batch takes it:
 * view-space t and column-major R, the winning hypothesis's fp64 model rounded to float. */
typedef struct mage_reloc_pnp_result {
    uint32_t verdict;       /* MAGE_RP_* */
    uint32_t status;        /* MAGE_RP_STATUS_* bits; with OVER_LIMIT or BAD_INDEX the problem has no other output */
    uint32_t n_matches;     /* the matches the stage ran on */
    uint32_t n_inliers;     /* the winner's inliers (maxGoodCount) */
    uint32_t n_in_front;    /* those RemoveMapPointsThatAreBehind leaves */
    uint32_t n_kept;        /* min(n_in_front, cap): the inlier indices written; the observations when OK */
    int32_t win_iteration;  /* the winner's RANSAC iteration, or -1 */
    int32_t win_indices[5]; /* its five matches in draw order */
    uint32_t iterations;    /* the final niters of the adaptive loop */
    uint32_t iterations_run; /* iterations the loop went through before it ended */
    float pos3[3], r9[9];
} mage_reloc_pnp_result;

/* Bytes of one problem's trace for `iterations` RANSAC iterations, arrays in this order:
 *   double R[iterations][9]      the hypothesis's rotation, row-major (zero without a model);
 *   double t[iterations][3]      its translation;
 *   double err[iterations][3]    the three EPnP starts' summed reprojection errors, -1 where a start failed;
 *   int32 indices[iterations][5] the sample's matches in draw order, or -1 five times (no sample);
 *   int32 solved[iterations]     1 when the sample gave a model;
 *   uint32 inliers[iterations]   its inlier count;
 * 148 bytes per iteration, the total rounded up to 8.  Every iteration is filled, also those the
 * adaptive loop did not reach.  With exactly five matches iteration 0 is the one solve on all of
 * them and the others hold no sample. */
uint64_t mage_reloc_pnp_trace_bytes(uint32_t iterations);

/* Bytes of mage_reloc_pnp_batch_device's scratch: the work buffer (problems traces, when no trace
 * is given), the gathered correspondences, one bit per match and hypothesis, the kept counts. */
uint64_t mage_reloc_pnp_scratch_bytes(uint32_t iterations, uint32_t problems, uint32_t match_cap, int32_t with_trace);

/* The PnP stage for `problems` (lost frame, candidate keyframe) problems, five launches on `stream`
 * with no host step between them:
 *   a. the limits and index checks, the MinBruteForceCorrespondences gate (:291), the
 *      correspondences gathered in match order (:301-308), the RANSAC sampler
 *      (RANSACPointSetRegistrator::getSubset);
 *   b. EPnP on five points per hypothesis;
 *   c. the inlier rule of every hypothesis over all matches;
 *   d. the adaptive loop replayed over the counts, the winner's inliers in match order,
 *      RemoveMapPointsThatAreBehind (:209-216), the RansacInliersPctRequired gate (:339), the result;
 *   e. d_obs_start (problems + 1 words, the prefix of the OK problems' kept counts) and the inputs of
 *      BundleAdjustPose as mage_ba_pose_batch_device takes them, compacted: per kept inlier the map
 *      point (d_points3), the keypoint (d_uv) and the map point's information value (d_info).
 * Per problem: d_intr4 4 floats {cx, cy, fx, fy} (the undistorted calibration); d_map_xyzi kf_pitch
 * x 4 floats, the candidate keyframe's keypoints' map points {x, y, z, information}, information
 * <= 0 marking a keypoint with no map point; d_kp kp_pitch keypoints of the current frame, d_n_kp
 * of them valid; d_matches match_cap records, d_n_matches of them valid, query_idx into the
 * candidate and train_idx into the current frame.  Outputs per problem: d_result; d_inlier_idx cap
 * match indices (n_kept written, for MAGE_RP_OK and MAGE_RP_FEW_INLIERS); d_pos3 / d_r9 the result's
 * pose (the identity unless a model was found).  d_points3 / d_uv / d_info hold problems x cap
 * entries at most.  d_trace: NULL, or problems x mage_reloc_pnp_trace_bytes(iterations) bytes.
 * d_scratch: mage_reloc_pnp_scratch_bytes(...) bytes, 256-byte aligned.  Nothing is written past a
 * problem's counts; a problem that stops in (a) leaves its trace untouched; the other problems are
 * unaffected.  mage_ba_pose_batch_device can be queued behind the stage on the same stream. */
mage_status mage_reloc_pnp_batch_device(const mage_reloc_settings* settings, uint32_t problems, const float* d_intr4,
                                        const float* d_map_xyzi, int64_t kf_pitch, const mage_keypoint* d_kp,
                                        int64_t kp_pitch, const uint32_t* d_n_kp, const mage_dmatch* d_matches,
                                        uint32_t match_cap, const uint32_t* d_n_matches, mage_reloc_pnp_result* d_result,
                                        uint32_t* d_inlier_idx, uint32_t cap, uint32_t* d_obs_start, float* d_points3,
                                        float* d_uv, float* d_info, float* d_pos3, float* d_r9, void* d_trace,
                                        void* d_scratch, mage_stream stream);

/* One problem, host buffers, synchronous, runs on `device`: map_xyzi n_kf x 4 floats, kp n_kp
 * keypoints; inlier_idx, points3, uv, info sized for cap entries (n_kept are written, the last three
 * for MAGE_RP_OK only); trace NULL or mage_reloc_pnp_trace_bytes(iterations) bytes. */
mage_status mage_reloc_pnp(const mage_reloc_settings* settings, const float* intr4, const float* map_xyzi, uint32_t n_kf,
                           const mage_keypoint* kp, uint32_t n_kp, const mage_dmatch* matches, uint32_t n_matches,
                           mage_reloc_pnp_result* result, uint32_t* inlier_idx, uint32_t cap, float* points3, float* uv,
                           float* info, void* trace, int device);

/* The same in plain C++ on the calling thread: the sequential loop of
 * RANSACPointSetRegistrator::run over the same arithmetic, the CPU backend, bit-identical to the
 * kernels.  Without a trace the hypotheses past the loop's end are not computed.  No GPU. */
mage_status mage_reloc_pnp_host(const mage_reloc_settings* settings, const float* intr4, const float* map_xyzi,
                                uint32_t n_kf, const mage_keypoint* kp, uint32_t n_kp, const mage_dmatch* matches,
                                uint32_t n_matches, mage_reloc_pnp_result* result, uint32_t* inlier_idx, uint32_t cap,
                                float* points3, float* uv, float* info, void* trace);

/* Test hooks of the adaptive loop.  _update: out[g] = RANSACUpdateNumIters(confidence, (n - g) / n,
 * 5, max_iters) for g in 0..n.  _loop: the loop over given outcomes (solved[i], inliers[i];
 * every iteration sampled) for n matches, with the replay the kernels run (sequential == 0) or the
 * twin's sequential loop; out = {winner or -1, its count, final niters, iterations run}. */
mage_status mage_debug_reloc_pnp_update(double confidence, uint32_t n, uint32_t max_iters, int32_t* out);
mage_status mage_debug_reloc_pnp_loop(const int32_t* solved, const uint32_t* inliers, uint32_t max_iters, uint32_t n,
                                      double confidence, int32_t sequential, int32_t* out);

/* ------------------------------------------------------------------------------------------ */
/* Relocalisation — the rest of TryEstimatePoseFromCandidates behind PNPRansac                  */
/* (Tracking/PoseEstimator.cpp:346-436): the first BundleAdjustPose, the guided search, the     */
/* second BundleAdjustPose, the gates around them and the choice of the candidate              */
/* ------------------------------------------------------------------------------------------ */

/* A problem's verdict. */
#define MAGE_RG_OK 0
#define MAGE_RG_SKIPPED 1            /* the PnP stage did not end MAGE_RP_OK, the frame has fewer keypoints than
                                        MinBruteForceCorrespondences (:233), the slot is past the frame's candidate
                                        count, or a status bit below stopped the problem */
#define MAGE_RG_FEW_RADIUS_MATCHES 2 /* matchCount < MinRadiusMatchCorrespondences (:391) */
#define MAGE_RG_FEW_MAP_POINTS 3     /* fewer than MinMapPoints left by RemoveMapPointsThatAreBehind (:406) */
#define MAGE_RG_FEW_BA_INLIERS 4     /* (n - outliers) / (float)n < BundleAdjustInliersPctRequired (:422) */

/* Bits of a problem's status word. */
#define MAGE_RG_STATUS_OVER_LIMIT 1u /* over 4096 keypoints on a side, or a count over its pitch */
#define MAGE_RG_STATUS_OVER_CAP 2u   /* more guided queries than `cap` (n_queries reports cap; the rest is dropped) */
#define MAGE_RG_STATUS_BAD_ORDER 4u  /* an order entry names no keypoint of the candidate, or one with no map point */

/* What the stage decides for one problem; written whole for every problem, zero (the poses the
 * identity) where a step was not reached.  Poses as mage_ba_pose_batch takes them. */
typedef struct mage_reloc_guided_result {
    uint32_t verdict;          /* MAGE_RG_* */
    uint32_t status;           /* MAGE_RG_STATUS_* bits; with OVER_LIMIT or BAD_ORDER the problem has no other output */
    uint32_t n_assoc;          /* the candidate's associations that were projected */
    uint32_t n_queries;        /* those with Distance >= 0 (:363): the RadiusMatch queries (at most cap) */
    uint32_t n_radius_matches; /* matchCount (:376) */
    uint32_t n_in_front;       /* the associations RemoveMapPointsThatAreBehind leaves (:405): n of the second BA */
    uint32_t n_outliers;       /* the second bundle adjustment's outliers */
    float pos3_first[3], r9_first[9]; /* the pose after the first BundleAdjustPose (:346-347) */
    float pos3[3], r9[9];             /* the pose after the second (:419); the frame's pose when MAGE_RG_OK */
} mage_reloc_guided_result;

/* The routine's outcome for one lost frame. */
typedef struct mage_reloc_frame_result {
    int32_t index;    /* indexOfSuccess: the lowest candidate whose pass succeeds, or -1 */
    uint32_t n_assoc; /* the associations the frame takes (that candidate's n_in_front), 0 without success */
    float pos3[3], r9[9]; /* the frame's pose (the identity without success) */
} mage_reloc_frame_result;

/* The stage's buffers.  struct_size must be sizeof(mage_reloc_guided_args).  The problems are laid
 * out frames x candidates_per_frame, problem = frame * candidates_per_frame + candidate; d_n_candidates
 * (one count per frame; NULL: candidates_per_frame each) tells how many of a frame's slots hold a
 * candidate.  Every per-problem array is indexed by problem, as the PnP stage's are: the lost
 * frame's keypoints, descriptors and intrinsics are repeated for each of its candidates.
 * Inputs: d_intr4 {cx, cy, fx, fy} of the lost frame (the projection, :358); d_ba_intr4 those of
 * the candidate for both bundle adjustments (:177), NULL = d_intr4; d_map_xyzi / d_kf_kp / d_kf_desc
 * kf_pitch entries of the candidate (map point {x, y, z, information}, keypoint, 32-byte
 * descriptor), d_n_kf valid; d_order NULL, or kf_pitch candidate keypoint indices per problem in
 * IterateAssociations' order, d_n_order of them valid (NULL order: ascending keypoint index over
 * those with information > 0); d_kp / d_desc kp_pitch entries of the lost frame, d_n_kp valid;
 * then the PnP stage's outputs as it left them.
 * Outputs per problem, `cap` entries each unless noted: the RadiusMatch queries (d_query_kp,
 * d_query_pos 2 floats, d_query_desc 32 bytes, d_query_ref the candidate keypoint) and their count
 * d_n_queries; d_radius_matches / d_n_radius as mage_radius_match_batch_device leaves them;
 * d_assoc {candidate keypoint, frame keypoint} per association (n_in_front written);
 * d_ba_obs_start (problems + 1) and d_ba_points3 / d_ba_uv / d_ba_info / d_ba_outlier the second
 * bundle adjustment's observations, compacted over the problems (problems x cap at most);
 * d_result; d_frame_result (one per frame); d_qt7_first / d_qt7 as mage_ba_pose_batch_device's
 * d_qt7_out, for every problem, those without observations included.  d_scratch: mage_reloc_guided_scratch_bytes(...) bytes,
 * 256-byte aligned. */
typedef struct mage_reloc_guided_args {
    uint32_t struct_size;
    uint32_t frames, candidates_per_frame, cap;
    uint32_t pnp_cap; /* the `cap` the PnP stage ran with: its observations per problem at most */
    int32_t pose_max_hamming_distance;   /* PoseEstimationSettings.OrbMatcherSettings.MaxHammingDistance 30 */
    int32_t pose_min_hamming_difference; /* ... MinHammingDifference 1 */
    int64_t kf_pitch, kp_pitch;
    const uint32_t* d_n_candidates;
    const float *d_intr4, *d_ba_intr4, *d_map_xyzi;
    const mage_keypoint* d_kf_kp;
    const uint8_t* d_kf_desc;
    const uint32_t* d_n_kf;
    const int32_t* d_order;
    const uint32_t* d_n_order;
    const mage_keypoint* d_kp;
    const uint8_t* d_desc;
    const uint32_t* d_n_kp;
    const mage_reloc_pnp_result* d_pnp_result;
    const uint32_t* d_obs_start;
    const float *d_points3, *d_uv, *d_info, *d_pos3, *d_r9;
    mage_keypoint* d_query_kp;
    float* d_query_pos;
    uint8_t* d_query_desc;
    int32_t* d_query_ref;
    uint32_t* d_n_queries;
    mage_dmatch* d_radius_matches;
    uint32_t* d_n_radius;
    int32_t* d_assoc;
    uint32_t* d_ba_obs_start;
    float *d_ba_points3, *d_ba_uv, *d_ba_info;
    uint8_t* d_ba_outlier;
    mage_reloc_guided_result* d_result;
    mage_reloc_frame_result* d_frame_result;
    double *d_qt7_first, *d_qt7; /* NULL, or 7 doubles per problem: the two bundle adjustments' fp64 poses */
    void* d_scratch;
} mage_reloc_guided_args;

/* Bytes of the stage's scratch for `problems` problems of `cap` entries behind a PnP stage of
 * `pnp_cap` observations per problem. */
uint64_t mage_reloc_guided_scratch_bytes(uint32_t problems, uint32_t cap, uint32_t pnp_cap);

/* The stage behind mage_reloc_pnp_batch_device on `stream`, no host step:
 *   a. mage_ba_pose_batch_device(bundle_adjust_iterations steps, Huber 1.8,
 *      max_bundle_adjust_reprojection_error unsquared as RunBundleAdjustment passes it) on the PnP
 *      stage's arrays: the first BundleAdjustPose (:346);
 *   b. the query kernel: limits, order and frame checks, ProjectUndistorted of the candidate's
 *      associations through the refined pose in float, Distance >= 0 kept in order (:351-371);
 *   c. mage_radius_match_batch_device at search_radius with the pose estimator's matcher settings;
 *   d. the gate kernel and the pack kernel: MinRadiusMatchCorrespondences (:391), the matches in
 *      query order as associations, RemoveMapPointsThatAreBehind (:405), MinMapPoints (:406); then
 *      d_ba_obs_start as the prefix of the counts and the second bundle adjustment's inputs;
 *   e. mage_ba_pose_batch_device again, with outliers (:419);
 *   f. the decide kernel, one workgroup per frame: the outlier counts, the
 *      BundleAdjustInliersPctRequired gate (:422), the result records and the frame's record.
 * The frame's record names the lowest candidate index whose pass succeeds: every round of the
 * reference's round-robin repeats the same RANSAC and everything behind it is a function of its
 * result, so for round_robin_iterations >= 1 that is indexOfSuccess; with 0 rounds it is -1.
 * Candidates behind the winner are computed and reported all the same, where the reference would
 * not have looked at them.  An OVER_LIMIT or BAD_ORDER problem gets its status bit and the identity
 * poses and nothing else of it is written; nothing is written past a problem's counts; the other
 * problems are unaffected.  Order entries are not checked for repeats.  The candidate's own gate
 * (:269, fewer associated keypoints than MinBruteForceCorrespondences) is not repeated: IndexedMatch
 * gives at most one match per associated keypoint, so the PnP stage's gate (:291) has stopped it. */
mage_status mage_reloc_guided_batch_device(const mage_reloc_settings* settings, const mage_reloc_guided_args* args,
                                           mage_stream stream);

/* One lost frame with n_candidates candidates, host buffers, synchronous, on `device`: the PnP
 * stage, then the stage above.  Candidate arrays are pitched by kf_pitch (map_xyzi, kf_kp, kf_desc,
 * order) and match_cap (matches); order / n_order / ba_intr4 may be NULL; ba_intr4 is 4 floats per
 * candidate.  Outputs: results and pnp_results (NULL allowed) n_candidates records, frame one
 * record, assoc n_candidates x cap x 2 (n_in_front pairs written per candidate, for every
 * candidate that reached the second bundle adjustment). */
mage_status mage_reloc_guided(const mage_reloc_settings* settings, int32_t pose_max_hamming_distance,
                              int32_t pose_min_hamming_difference, uint32_t n_candidates, const float* intr4,
                              const float* ba_intr4, const float* map_xyzi, const mage_keypoint* kf_kp,
                              const uint8_t* kf_desc, uint32_t kf_pitch, const uint32_t* n_kf, const int32_t* order,
                              const uint32_t* n_order, const mage_keypoint* kp, const uint8_t* desc, uint32_t n_kp,
                              const mage_dmatch* matches, uint32_t match_cap, const uint32_t* n_matches, uint32_t cap,
                              mage_reloc_guided_result* results, mage_reloc_pnp_result* pnp_results,
                              mage_reloc_frame_result* frame, int32_t* assoc, int device);

/* What mage_reloc_candidates_batch_device needs on top of mage_reloc_guided_args: per problem the
 * BoW leaves of the candidate's (kf_pitch) and of the lost frame's (kp_pitch) descriptors, the
 * candidate's associated-keypoint mask (kf_pitch bytes, GetAssociatedKeypointMask), and the buffers
 * IndexedMatch and the PnP stage write: d_matches problems x match_cap with d_n_matches, d_match_status
 * one word (mage_indexed_match_batch_device's; zeroed by the call), then the PnP stage's outputs and
 * scratch as mage_reloc_pnp_batch_device takes them with cap = match_cap and no trace.
 * struct_size must be sizeof(mage_reloc_candidates_args). */
typedef struct mage_reloc_candidates_args {
    uint32_t struct_size;
    uint32_t match_cap;
    const uint32_t *d_leaf_kf, *d_leaf;
    const uint8_t* d_mask_kf;
    mage_dmatch* d_matches;
    uint32_t *d_n_matches, *d_match_status;
    mage_reloc_pnp_result* d_pnp_result;
    uint32_t *d_inlier_idx, *d_obs_start;
    float *d_points3, *d_uv, *d_info, *d_pos3, *d_r9;
    void* d_pnp_scratch;
} mage_reloc_candidates_args;

/* The routine from IndexedMatch on (:279-436) on `stream`, no host step:
 * mage_indexed_match_batch_device (A = the candidate under its associated-keypoint mask, B = the lost
 * frame, the relocaliser's OrbMatcherSettings), mage_reloc_pnp_batch_device on its matches, then
 * mage_reloc_guided_batch_device.  `guided` is filled as for that call except its PnP-stage fields
 * (d_pnp_result, d_obs_start, d_points3, d_uv, d_info, d_pos3, d_r9, pnp_cap), which are taken from
 * `cand`.  A problem with more matches than match_cap is the PnP stage's OVER_LIMIT and so SKIPPED. */
mage_status mage_reloc_candidates_batch_device(const mage_reloc_settings* settings, const mage_reloc_candidates_args* cand,
                                               const mage_reloc_guided_args* guided, mage_stream stream);

/* The twin in plain C++ for one problem, no GPU, byte-identical to the kernels phase by phase.  The
 * library has no host pose bundle adjustment and no host RadiusMatch, so their outcomes are inputs.
 *   1. from the first refined pose (pos3_first, r9_first) and pnp_ok (the PnP stage ended
 *      MAGE_RP_OK without a stopping status bit): the checks and the query set (query_* / n_queries);
 *   2. radius_matches != NULL: the gates, the association records and the second bundle
 *      adjustment's inputs (n_in_front entries);
 *   3. outlier != NULL (n_in_front flags) with pos3_second / r9_second: the final record.
 * A NULL stops after the phase before it; *result is what the kernels hold at that point. */
mage_status mage_reloc_guided_host(const mage_reloc_settings* settings, int32_t pnp_ok, const float* intr4,
                                   const float* map_xyzi, const mage_keypoint* kf_kp, const uint8_t* kf_desc,
                                   uint32_t n_kf, const int32_t* order, uint32_t n_order, const mage_keypoint* kp,
                                   uint32_t n_kp, const float* pos3_first, const float* r9_first, uint32_t cap,
                                   mage_reloc_guided_result* result, mage_keypoint* query_kp, float* query_pos,
                                   uint8_t* query_desc, int32_t* query_ref, const mage_dmatch* radius_matches,
                                   uint32_t n_radius_matches, int32_t* assoc, float* ba_points3, float* ba_uv,
                                   float* ba_info, const uint8_t* outlier, const float* pos3_second,
                                   const float* r9_second);

/* The frame's record from its candidates' records (the decide kernel's last step). */
mage_status mage_reloc_guided_choose_host(const mage_reloc_settings* settings, const mage_reloc_guided_result* results,
                                          uint32_t n_candidates, mage_reloc_frame_result* frame);

/* ------------------------------------------------------------------------------------------ */
/* Scene extent — CalculateBoundingPlaneDepthsForKeyframe (Tracking/BoundingPlaneDepths.cpp:    */
/* 16-87): a tracked frame's near and far plane depths and its sparse depth map                */
/* ------------------------------------------------------------------------------------------ */

/* BoundingDepthSettings (MageSettings.h:216-223) in the reference's order.  struct_size must be
 * sizeof(mage_bounding_depth_settings).  Both softness values must lie in [0, 1): the reference
 * would index past the end of its depth list with anything else (MAGE_EINVAL here). */
typedef struct mage_bounding_depth_settings {
    uint32_t struct_size;
    float region_of_interest_min_x; /* RegionOfInterestMinX 0.1, a share of the image width */
    float region_of_interest_min_y; /* RegionOfInterestMinY 0.1 */
    float region_of_interest_max_x; /* RegionOfInterestMaxX 0.9 */
    float region_of_interest_max_y; /* RegionOfInterestMaxY 0.9 */
    float near_depth_softness;      /* NearDepthSoftness 0: the share of the valid depths ruled out at the near end */
    float far_depth_softness;       /* FarDepthSoftness 0 */
} mage_bounding_depth_settings;

#define MAGE_INVALID_DEPTH (-1.0f) /* Depth::INVALID_DEPTH (Data/Data.h:390) */
#define MAGE_BD_MAX_POINTS 8192u   /* map points per frame: the depth list is 32 KB of LDS */

/* Bits of a frame's status word. */
#define MAGE_BD_STATUS_BAD_INDEX 1u   /* a keypoint index outside the frame's count: the point contributes no valid
                                         depth, its sparse record is still written */
#define MAGE_BD_STATUS_NONPOSITIVE 2u /* a valid depth that is not > 0 (the reference asserts, :50); values reported all the same */
#define MAGE_BD_STATUS_OVER_LIMIT 4u  /* n_points over `cap`, or `cap` over MAGE_BD_MAX_POINTS: the record is
                                         {-1, -1, 0, n_points} and nothing else of the frame is written */

/* ProjectedPoint (Data/Data.h:112-124), 16 bytes: a map point through ProjectUndistorted
 * (Tracking/Reprojection.cpp:26-42; a camera-space depth of exactly 0 divides by 1) and its id. */
typedef struct mage_projected_point {
    float x, y, depth;
    int32_t id;
} mage_projected_point;

/* InternalDepth without its sparse map, 20 bytes. */
typedef struct mage_depth_result {
    float near_plane; /* NearPlaneDepth, MAGE_INVALID_DEPTH when near > far (no valid depth) */
    float far_plane;  /* FarPlaneDepth */
    uint32_t n_valid; /* points whose keypoint lies inside the closed region of interest */
    uint32_t n_points;
    uint32_t status;  /* MAGE_BD_STATUS_* bits */
} mage_depth_result;

/* One frame on the calling thread in plain C++, the CPU backend, bit-identical to the kernel.  The
 * pose is the view matrix in the bundler form (pos3 view-space t, r9 column-major R), intr4 = {cx,
 * cy, fx, fy} of the undistorted calibration.  The world position c and forward f are column 3 and
 * column 2 of Utils/cv.h Invert(view) (Data/Pose.cpp:110-118), c formed as -(R^T t) the way the
 * third-frame stage forms camera centres: cv::Matx's product differs in the sign of a zero only.
 * Point i is map_xyzi[4 i .. 4 i + 3] = {x, y, z, the id's 32 bits} and is associated with keypoint
 * kp_index[i] of the frame's n_kp keypoints.  With the region bounds min/max x = share * width and
 * min/max y = share * height as float products, a point whose keypoint lies inside the closed region
 * adds depth = (p - c) . f to the valid depths; every point gets sparse[i] in point order.
 * near_plane is the valid depth of rank (size_t)(near_depth_softness * n_valid) in ascending order,
 * far_plane the one of rank (size_t)(far_depth_softness * n_valid) in descending order, the product
 * taken in float, a rank that rounds up to n_valid held at n_valid - 1; depths compare under the
 * total order of their bit patterns in which -0 < +0, so any exact selection gives the same bits.
 * Without a valid depth near stays FLT_MAX and far FLT_MIN (the smallest positive normal, the
 * reference's start value), near > far, and both become MAGE_INVALID_DEPTH; so they do when the two
 * softness values make the ranks cross.  `cap` is what `sparse` holds. */
mage_status mage_bounding_plane_depths_host(const mage_bounding_depth_settings* settings, const float* pos3,
                                            const float* r9, const float* intr4, uint32_t width, uint32_t height,
                                            const mage_keypoint* kp, uint32_t n_kp, const float* map_xyzi,
                                            const int32_t* kp_index, uint32_t n_points, uint32_t cap,
                                            mage_depth_result* result, mage_projected_point* sparse);

/* The same through the kernel: host buffers, synchronous, on `device`. */
mage_status mage_bounding_plane_depths(const mage_bounding_depth_settings* settings, const float* pos3, const float* r9,
                                       const float* intr4, uint32_t width, uint32_t height, const mage_keypoint* kp,
                                       uint32_t n_kp, const float* map_xyzi, const int32_t* kp_index, uint32_t n_points,
                                       uint32_t cap, mage_depth_result* result, mage_projected_point* sparse, int device);

/* `frames` frames in one launch on `stream`, one workgroup per frame: the projection and the region
 * test by the threads, the two order statistics by a radix selection over the depth list in LDS.
 * Per frame f: d_pos3 3, d_r9 9, d_intr4 4 floats; d_size {width, height}; d_kp kp_pitch keypoints,
 * d_n_kp[f] of them valid (a count over kp_pitch is read as kp_pitch); d_map_xyzi point_pitch x 4
 * floats and d_kp_index point_pitch words, d_n_points[f] of them valid; d_result one record;
 * d_sparse point_pitch records, d_n_points[f] written.  cap <= point_pitch.  Nothing is written past
 * a frame's counts; an OVER_LIMIT frame gets its record only; the other frames are unaffected.
 * d_result can be read by index by a later stage on the same stream. */
mage_status mage_bounding_plane_depths_batch_device(const mage_bounding_depth_settings* settings, uint32_t frames,
                                                    const float* d_pos3, const float* d_r9, const float* d_intr4,
                                                    const uint32_t* d_size, const mage_keypoint* d_kp, int64_t kp_pitch,
                                                    const uint32_t* d_n_kp, const float* d_map_xyzi,
                                                    const int32_t* d_kp_index, int64_t point_pitch,
                                                    const uint32_t* d_n_points, uint32_t cap, mage_depth_result* d_result,
                                                    mage_projected_point* d_sparse, mage_stream stream);

/* ------------------------------------------------------------------------------------------ */
/* Scene extent — CalculateVolumeOfInterest (VolumeOfInterest/VolumeOfInterest.cpp:45-259)     */
/* behind MAGESlam::TryGetVolumeOfInterest (MageSlam.h:119, 178; Map/PoseHistory.cpp:58-75)    */
/* ------------------------------------------------------------------------------------------ */

/* VolumeOfInterestSettings (MageSettings.h:290-307) in the reference's order, then the constants
 * mage_voi_settings_prepare derives from them.  struct_size must be sizeof(mage_voi_settings);
 * iterations must be in 0..MAGE_VOI_MAX_ITERATIONS.  Every entry below derives the constants again
 * on a copy, so a caller need not prepare. */
typedef struct mage_voi_settings {
    uint32_t struct_size;
    float threshold;             /* Threshold 0.5 */
    int32_t iterations;          /* Iterations 3 */
    int32_t voxel_count_floor;   /* VoxelCountFloor 16000 */
    float away_prominence;       /* AwayProminence 1.2 */
    float toward_prominence;     /* TowardProminence 0.1 */
    float side_prominence;       /* SideProminence 1 */
    float kernel_angle_x_rads;   /* KernelAngleXRads deg2rad(60) */
    float kernel_angle_y_rads;   /* KernelAngleYRads deg2rad(40) */
    float kernel_pitch_rads;     /* KernelPitchRads 0 */
    float kernel_roll_rads;      /* KernelRollRads 0 */
    float kernel_yaw_rads;       /* KernelYawRads deg2rad(5) */
    float kernel_depth_modifier; /* KernelDepthModifier 1 */
    float kernel_rotation[9];    /* derived: ToMat(pitch, roll, yaw) (Utils/cv.h:96-116), row-major */
    float tan_min_angle;         /* derived: tan(min(angle x, angle y)) (:59) */
    float tan_half_angle_x;      /* derived: tan(angle x / 2) (:103) */
    float tan_half_angle_y;      /* derived: tan(angle y / 2) (:104) */
} mage_voi_settings;

#define MAGE_VOI_MAX_ITERATIONS 30
#define MAGE_VOI_OK 0
#define MAGE_VOI_NO_KEYFRAMES 1 /* the reference returns false; the bounds and the trace are untouched */
#define MAGE_VOI_DEGENERATE 2   /* a level with voxelCount == 0, a diagonal that is <= 0 or not finite, a dims product
                                   over 2^31 - 1, or a voxel value that is not finite */
#define MAGE_VOI_EMPTY 3        /* nothing passed a level's threshold */

/* The outcome of one problem.  The level loop stops at the first DEGENERATE or EMPTY level and the
 * bounds hold what the level before left (the frustum box when the first level stops). */
typedef struct mage_voi_result {
    float min[3], max[3];
    uint32_t status;      /* MAGE_VOI_* */
    uint32_t levels_done;
} mage_voi_result;

/* One level's trace record, 60 bytes; a problem has `iterations` of them, zeroed first and filled as
 * far as the level got (a level that is DEGENERATE by its grid stays zero; one with a voxel value
 * that is not finite has side, dims, voxel_min and voxel_max). */
typedef struct mage_voi_level {
    float side;                   /* voxelSideLength */
    int32_t dims[3];
    float voxel_min, voxel_max;   /* minVoxelValue / maxVoxelValue after the level: they run on across the levels */
    float threshold;
    float box_min[3], box_max[3]; /* the level's resulting box */
    uint32_t n_voxels;            /* voxels strictly above the threshold */
    uint32_t n_centroids;         /* keyframe centroids whose stored score is above it */
} mage_voi_level;

/* Fills the derived constants with libm on the host (sinf, cosf, tanf, as the reference calls them). */
mage_status mage_voi_settings_prepare(mage_voi_settings* settings);

/* TeardropScore (:63-86) of n_points points {x, y, z} against n_kf keyframes: scores[p * n_kf + k].
 * Keyframes as below.  The twin's own function. */
mage_status mage_voi_teardrop_host(const mage_voi_settings* settings, const float* kf_world, const float* near_far,
                                   uint32_t n_kf, const float* points, uint32_t n_points, float* scores);

/* One problem (one pose history) on the calling thread in plain C++, bit-identical to the kernels.
 * kf_world: n_kf world-from-camera matrices, 3 x 4 row-major (the inverse view matrix that
 * ToPose(WorldPosition) holds).  The keyframes' depths are near_far (n_kf pairs {near, far}), or with
 * near_far NULL the records depth_records[depth_index[k]] of the depth stage (an index outside
 * n_depth_records reads as MAGE_INVALID_DEPTH for both).  A depth of -1 is passed through as the
 * reference passes it.  trace: NULL, or `iterations` records.
 * Follows VolumeOfInterest.cpp in float with these deviations: acos, exp and the cube root are the
 * library's own (csrc/scene_math.hpp; acos clamps its argument to [-1, 1]; the reference writes
 * pow(v, 1.f / 3.f)); minima and maxima are taken under the total order in which -0 < +0; the
 * status replaces undefined arithmetic.  The maxima start at numeric_limits<float>::min() as the
 * reference's do, so a maximum never drops below about 1.2e-38. */
mage_status mage_volume_of_interest_host(const mage_voi_settings* settings, const float* kf_world, const float* near_far,
                                         const mage_depth_result* depth_records, uint32_t n_depth_records,
                                         const uint32_t* depth_index, uint32_t n_kf, mage_voi_result* result,
                                         mage_voi_level* trace);

/* The same through the kernels: host buffers, synchronous, on `device`. */
mage_status mage_volume_of_interest(const mage_voi_settings* settings, const float* kf_world, const float* near_far,
                                    const mage_depth_result* depth_records, uint32_t n_depth_records,
                                    const uint32_t* depth_index, uint32_t n_kf, mage_voi_result* result,
                                    mage_voi_level* trace, int device);

/* Bytes of mage_volume_of_interest_batch_device's scratch: per problem the keyframes' records and
 * scores and the levels' accumulators.  Voxel values are not kept: the threshold pass computes them
 * again. */
uint64_t mage_volume_of_interest_scratch_bytes(uint32_t problems, uint32_t kf_pitch);

/* `problems` problems as one chain of launches on `stream` with no host step: a setup launch (the
 * keyframes' records, the frustum box, the keyframe scores), two launches per level (the voxel
 * values' minimum and maximum; the threshold and the next box) and a closing launch that writes
 * the last level's outcome.  A fixed number of workgroups per problem walks the voxels with a
 * grid-stride loop over the count each workgroup derives from the box; the keyframes' records are
 * staged through LDS in chunks, so n_kf is unbounded.  Per problem: d_kf_world kf_pitch matrices,
 * d_n_kf valid (a count over kf_pitch is read as kf_pitch); d_near_far kf_pitch pairs, or NULL and
 * d_depth_index kf_pitch indices into the one array d_depth_records of n_depth_records records (the
 * depth stage's d_result, on the same stream); d_result one record; d_trace NULL or `iterations`
 * records; d_scratch 256-byte aligned. */
mage_status mage_volume_of_interest_batch_device(const mage_voi_settings* settings, uint32_t problems,
                                                 const float* d_kf_world, int64_t kf_pitch, const uint32_t* d_n_kf,
                                                 const float* d_near_far, const mage_depth_result* d_depth_records,
                                                 uint32_t n_depth_records, const uint32_t* d_depth_index,
                                                 mage_voi_result* d_result, mage_voi_level* d_trace, void* d_scratch,
                                                 mage_stream stream);

/* ------------------------------------------------------------------------------------------ */
/* Local bundle adjustment — replaces BundlerLib (Dependencies/BundlerLib/Include/BundlerLib.h) */
/* ------------------------------------------------------------------------------------------ */

typedef struct mage_ba mage_ba;

/* BundlerLib::BundlerLib(BundlerParameters{ArePointsFixed}) (BundlerLib.cpp:184-196). */
mage_status mage_ba_create(int32_t points_fixed, int device, mage_ba** out);
mage_status mage_ba_destroy(mage_ba* ba);

/* AllocateCameras + SetCameraPose for all cameras (BundlerLib.cpp:198-207, 261-278).
 * pos3: view-space position t (3 floats/camera); R9: rotation, Eigen column-major
 * (9 floats/camera); intr4: {cx, cy, fx, fy}; fixed: 0/1.  Only fx is used as the focal
 * length, as in the reference (CameraParameters(intr[2], (intr[0], intr[1]), 0)). */
mage_status mage_ba_set_cameras(mage_ba* ba, uint32_t n, const float* pos3, const float* r9,
                                const float* intr4, const uint8_t* fixed);
/* FixCameraPose (BundlerLib.cpp:280-283). */
mage_status mage_ba_fix_camera(mage_ba* ba, uint32_t idx, int32_t fixed);
/* AllocateMapPoints + SetMapPoint (BundlerLib.cpp:209-217, 285-292). */
mage_status mage_ba_set_points(mage_ba* ba, uint32_t n, const float* xyz);
/* AllocateObservations + SetObservation (BundlerLib.cpp:219-229, 294-309). */
mage_status mage_ba_set_observations(mage_ba* ba, uint32_t n, const float* uv,
                                     const uint32_t* cam, const uint32_t* pt,
                                     const float* info);
/* SetCurrentLambda / GetCurrentLambda (BundlerLib.cpp:354-362). */
mage_status mage_ba_set_lambda(mage_ba* ba, float lambda);
mage_status mage_ba_get_lambda(mage_ba* ba, float* lambda);
/* Tether constraints: Allocate*Constraints(n) + Set*Constraint(i, ...) for one kind
 * (BundlerLib.cpp:229-257, 311-350; called from BundleAdjust.cpp:155-189).  Replaces the set of
 * that kind; the others are kept.  params per tether:
 *   MAGE_TETHER_DISTANCE  (SetFixedDistanceConstraint)     1 float: distance
 *   MAGE_TETHER_ROTATION  (SetRelativeRotationConstraint)  4 floats: quaternion x, y, z, w
 *   MAGE_TETHER_TRANSFORM (SetRelativeTransformConstraint) 7 floats: position x, y, z, then
 *                                                          quaternion x, y, z, w
 * weight[i] is the constraint weight.  Camera indices must be < the camera count and distinct
 * (MAGE_EINVAL otherwise); set the cameras first. */
enum { MAGE_TETHER_DISTANCE = 0, MAGE_TETHER_ROTATION = 1, MAGE_TETHER_TRANSFORM = 2 };
mage_status mage_ba_set_tethers(mage_ba* ba, uint32_t kind, uint32_t n, const uint32_t* cam1,
                                const uint32_t* cam2, const float* params, const float* weight);

/* StepBundleAdjustment (BundlerLib.cpp:364-447): one LM iteration per entry of huber[],
 * stopping early if an iteration fails; then the outlier / cheirality pass.  Outlier
 * observation indices are appended in ascending order (g2o active-edge order) to
 * outliers[0..cap); *n_out = number reported.  *mean_sq = Σ‖e‖²/count over kept edges
 * (NaN if none, as the reference's 0/0). */
mage_status mage_ba_step(mage_ba* ba, const float* huber, uint32_t nsteps,
                         float max_error_square, uint32_t* outliers, uint32_t cap,
                         uint32_t* n_out, float* mean_sq);

/* GetPose / GetPoint (BundlerLib.cpp:457-471), all at once. */
mage_status mage_ba_get_poses(mage_ba* ba, float* pos3, float* r9);
mage_status mage_ba_get_points(mage_ba* ba, float* xyz);

/* The fp64 estimate itself: qt7 = {qx, qy, qz, qw, tx, ty, tz} per camera, xyz per point
 * (either may be NULL).  Used by the parity tests; the reference exposes only the float casts. */
mage_status mage_ba_get_state_f64(mage_ba* ba, double* qt7, double* xyz);

/* Instrumentation: counters since creation. */
typedef struct mage_ba_stats {
    uint64_t iterations;      /* LM solve() calls */
    uint64_t trials;          /* LM inner trials (linear solves) */
    uint64_t rejected_trials; /* trials that popped the state */
    double last_chi2;         /* robust chi2 after the last iteration */
    double lambda;            /* current LM lambda */
} mage_ba_stats;
mage_status mage_ba_get_stats(mage_ba* ba, mage_ba_stats* stats);

/* Batched pose-only BA: TrackLocalMap::OptimizeCameraPose (TrackLocalMap.cpp:421-501) for many
 * independent frames in one launch.  Problem k = a fresh BundlerLib with ArePointsFixed, camera 0 =
 * (pos3[k], r9[k] column-major, intr4[k] = {cx, cy, fx, fy}, not fixed), observations obs_start[k] ..
 * obs_start[k+1]-1 each on its own fixed map point (points3, uv, info = MapPointRefinementConfidence),
 * then StepBundleAdjustment(nsteps x huber, max_error_square).  Outputs per problem: GetPose(0)
 * (pos3_out, r9_out column-major), mean_sq (the post-pass mean, NaN if nothing kept), optionally
 * qt7_out (fp64 q xyzw + t) and stats {LM iterations, trials}; per observation outlier = 1 where
 * the post-pass rejects it (outlierIndices = the flagged indices, ascending).  Host buffers,
 * synchronous; _device: device buffers, asynchronous on `stream`. */
mage_status mage_ba_pose_batch(uint32_t problems, const float* pos3, const float* r9, const float* intr4,
                               const uint32_t* obs_start, const float* points3, const float* uv, const float* info,
                               uint32_t nsteps, float huber, float max_error_square, float* pos3_out, float* r9_out,
                               double* qt7_out, uint8_t* outlier, float* mean_sq, uint32_t* stats, int device);
mage_status mage_ba_pose_batch_device(uint32_t problems, const float* d_pos3, const float* d_r9, const float* d_intr4,
                                      const uint32_t* d_obs_start, const float* d_points3, const float* d_uv,
                                      const float* d_info, uint32_t nsteps, float huber, float max_error_square,
                                      float* d_pos3_out, float* d_r9_out, double* d_qt7_out, uint8_t* d_outlier,
                                      float* d_mean_sq, uint32_t* d_stats, mage_stream stream);

/* ---------------------------------------------------------------------------------------------
 * C4 tracking loop (native host code over mage_radius_match + mage_ba_pose_batch): per frame the
 * constant-velocity prediction, ProjectUndistorted of the reference keyframe's map points and
 * RadiusMatch at SearchRadius / WiderSearchRadius / ExtraWiderSearchRadius
 * (PoseEstimator::TryEstimatePoseFromKeyframe, Core/MAGESLAM/Source/Tracking/PoseEstimator.cpp:
 * 439-607), TrackLocalMap's two OptimizeCameraPose passes (TrackLocalMap.cpp:37-140) and the
 * keyframe decision of NewKeyFrameDecision.cpp:196.  A keyframe's map points are its keypoints
 * back-projected onto the plane Z = plane_z (the reference triangulates; outside the hot path).
 * Same specification, expression by expression, as mageslam_amd/tracking.py's `track`.
 * --------------------------------------------------------------------------------------------- */
typedef struct mage_track_settings {
    float search_radius, wider_search_radius, extra_wider_search_radius; /* 12, 24, 36 px */
    double small_match_ratio;                                            /* FeatureSmallMatchRatioThreshold */
    uint32_t min_matches;
    int32_t max_hamming, min_hamming_difference;                         /* 30, 1 */
    uint32_t initial_steps;                                              /* 3 */
    float initial_huber;                                                 /* 4 */
    double initial_max_error;                                            /* 6 (squared inside) */
    uint32_t final_steps;                                                /* 4 */
    float final_huber;                                                   /* 0.9 */
    double final_max_error;                                              /* 4.5 */
    /* FIXED (deprecated; kept for ABI layout): must equal MapPointRefinementConfidence(0) =
     * 1 - 1/1.5^2, else MAGE_EINVAL.  Observation information now follows each map point's own
     * refinement count (MappingMath.h:42-49); the field will be dropped at the next ABI bump. */
    float refinement_info;
    double keyframe_ratio;                                               /* 0.5 */
    uint32_t keyframe_min;                                               /* 25 */
    /* TrackLocalMap's local-map search between the two pose passes (TrackLocalMap.cpp:114-265,
     * TrackLocalMapSettings MageSettings.h:180-194); local_map_keyframes = 0 turns it off.  The
     * local map is the last local_map_keyframes keyframes, visited in ascending keyframe id. */
    uint32_t local_map_keyframes;                                        /* 4 (<= 8) */
    float match_search_radius;                                           /* MatchSearchRadius 8 */
    int32_t local_max_hamming, local_min_hamming_difference;             /* OrbMatcherSettings 30, 1 */
    float min_view_cos;         /* cosf(deg2rad(MinDegreesBetweenCurrentViewAndMapPointView = 60)) */
    float image_border;                                                  /* PatchSize / 2 = 7.5 */
    uint32_t min_tracked;                                                /* MinTrackedFeatureCount 20 */
    float scale_factor;                                                  /* pyramid ScaleFactor 1.5 */
    uint32_t num_levels;                                                 /* pyramid levels 1 */
    int32_t width, height;                                               /* image size */
    /* Local bundle adjustment after every new keyframe (MappingWorker.cpp:228-371; device loop
     * only, mage_track_sequence refuses it): over the local map's keyframes, the free ones and the
     * points they observe chosen as GetMapPointsAndDistantKeyframes does (ThreadSafeMap.cpp:
     * 888-957, see ba_free_keyframes), every alive association of those points; one
     * StepBundleAdjustment per keyframe at MaxOutlierError with the persisted lambda and
     * covisibility threshold (tracking.py local_bundle_adjust). */
    uint32_t local_ba;                                                   /* 0: off */
    float ba_huber, ba_huber_scale, ba_max_outlier_error;                /* 1.8, 0.95, 7.25 */
    uint32_t ba_steps_per_run;                                           /* NumStepsPerRun 1 */
    float ba_low_connectivity_scale;                                     /* 1.5 */
    uint32_t ba_upper_connections;                                       /* UpperConnectionsForBA 2000 */
    float min_lambda;                                                    /* MappingSettings::MinLambda 1e-3 */
    /* 0 (default): the new keyframe Ki and the keyframes sharing >= theta map points with it are
     * free, every other observer and the sequence's first keyframe fixed; theta starts at
     * covis_min_threshold, steps by covis_ba_step while the associations lie outside
     * [ba_lower_connections, ba_upper_connections] (covis_max_steps + 1 rounds) and persists
     * across windows.  N > 0: the newest N keyframes of the window free, the older ones fixed. */
    uint32_t ba_free_keyframes;
    uint32_t covis_min_threshold;                                        /* CovisMinThreshold 15 */
    uint32_t covis_ba_step;                                              /* CovisBaStepThreshold 15 */
    uint32_t ba_lower_connections;                                       /* LowerConnectionsForBA 1500 */
    uint32_t covis_max_steps;                                            /* MaxSteps 1 */
    /* New map points' depth x (1 + sigma g), g a seeded unit-variance variate per (keyframe frame,
     * keypoint) (tracking.py depth_noise_factor): a triangulated point's depth error instead of the
     * plane back-projection's exact depth.  0: exact. */
    float map_point_depth_noise;
} mage_track_settings;

/* Features of `frames` frames (host): keypoints kp[frame_start[f] .. frame_start[f+1]) and their
 * descriptors (32 B each); K = {fx, fy, cx, cy}; first_pose = R (row-major, world -> camera) and
 * t of frame 0 (its keyframe).  Outputs per frame: poses (R row-major + t, 12 doubles), the
 * RadiusMatch count, the inliers after both passes (0 when lost) and the keyframe flag. */
mage_status mage_track_sequence(const mage_keypoint* kp, const uint8_t* desc, const uint32_t* frame_start,
                                uint32_t frames, const double K[4], const double first_pose[12], double plane_z,
                                const mage_track_settings* settings, double* poses, uint32_t* matches,
                                uint32_t* inliers, uint8_t* keyframe, int device);

/* The same loop device-resident (csrc/track.hip): features in device memory as the batched
 * extraction leaves them — frame f's keypoints at d_kp + f*pitch (pitch <= 4096), descriptors at
 * d_desc + 32*f*pitch, count d_n[f]; every per-frame decision (fallback radii, lost frames,
 * keyframes) is taken on the device, the host enqueues all frames on `stream` and synchronises
 * once.  Outputs (host) as mage_track_sequence, identical to it. */
mage_status mage_track_sequence_device(const mage_keypoint* d_kp, const uint8_t* d_desc, uint32_t pitch,
                                       const uint32_t* d_n, uint32_t frames, const double K[4],
                                       const double first_pose[12], double plane_z,
                                       const mage_track_settings* settings, double* poses, uint32_t* matches,
                                       uint32_t* inliers, uint8_t* keyframe, uint32_t* ba_outliers,
                                       mage_stream stream);

#ifdef __cplusplus
}
#endif

#endif /* MAGE_HOT_H */
