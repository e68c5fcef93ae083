// mage.hpp — header-only C++ facades over the C-ABI (include/mage_hot.h) with the reference's
// class shapes, so MAGE-SLAM's L3 callers (ImageAnalyzer, MapInitialization, BundleAdjust,
// TrackLocalMap) can switch by swapping the type they hold.  No OpenCV / Eigen / g2o types:
// keypoints are cv::KeyPoint-layout records, descriptors 32-byte rows, matrices plain floats
// in the reference's layouts (Eigen column-major rotations).  Errors throw like the reference:
// MAGE_EINVAL -> std::invalid_argument (CV_Assert), everything else -> mage::hot::Error.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../mage_hot.h"

namespace mage {
namespace hot {

struct Error : std::runtime_error {
    mage_status status;
    Error(mage_status s, const std::string& m) : std::runtime_error(m), status(s) {}
};

inline void check(mage_status s)
{
    if (s == MAGE_OK) return;
    std::string msg = mage_last_error();
    if (s == MAGE_EINVAL) throw std::invalid_argument(msg);
    throw Error(s, msg);
}

using KeyPoint = mage_keypoint;
using DMatch = mage_dmatch;
using Descriptor = std::array<uint8_t, 32>;  // ORBDescriptor (ORBDescriptor.h:14-133)

// OrbDetector (Core/MAGESLAM/Source/Image/OpenCVModified.h:64-173).
class OrbDetector {
public:
    OrbDetector(unsigned gaussianKernelSize, unsigned nfeatures, float scaleFactor, unsigned nlevels,
                unsigned patchSize, unsigned fastThreshold, bool useOrientation, float featureFactorANMS,
                float featureStrengthANMS, int strongResponseANMS, float minRobustFactor,
                float maxRobustFactor, int numCellsX, int numCellsY, int device = 0)
        : m_settings{gaussianKernelSize, nfeatures, scaleFactor, nlevels, patchSize, fastThreshold,
                     useOrientation ? 1 : 0, featureFactorANMS, featureStrengthANMS, strongResponseANMS,
                     minRobustFactor, maxRobustFactor, numCellsX, numCellsY}
    {
        check(mage_orb_create(&m_settings, device, &m_handle));
    }
    ~OrbDetector() { mage_orb_destroy(m_handle); }
    OrbDetector(const OrbDetector&) = delete;
    OrbDetector& operator=(const OrbDetector&) = delete;

    // DetectAndCompute(thread_memory, ImageData&, const cv::Mat&): the ImageData becomes the two
    // output vectors; `capacity` is ImageData's maxFeatures (defaults to nfeatures).
    void DetectAndCompute(const uint8_t* gray, int width, int height, int stride,
                          std::vector<KeyPoint>& keypoints, std::vector<Descriptor>& descriptors,
                          uint32_t capacity = 0)
    {
        const uint32_t cap = capacity ? capacity : m_settings.nfeatures;
        keypoints.resize(cap);
        descriptors.resize(cap);
        uint32_t n = 0;
        check(mage_orb_detect_and_compute(m_handle, gray, width, height, stride, keypoints.data(),
                                          descriptors.empty() ? nullptr : descriptors.front().data(), cap, &n));
        keypoints.resize(n);
        descriptors.resize(n);
    }

    mage_orb* handle() const { return m_handle; }

private:
    mage_orb_settings m_settings;
    mage_orb* m_handle = nullptr;
};

// GetDescriptorDistance (Core/MAGESLAM/Source/Tracking/FeatureMatcher.cpp:453-504).
inline int GetDescriptorDistance(const Descriptor& a, const Descriptor& b)
{
    return mage_hamming_distance(a.data(), b.data());
}

// Match (FeatureMatcher.cpp:61-190) with descriptor rows and boolean masks instead of
// AnalyzedImage; returns the match count and fills goodMatches (ascending A index).
inline unsigned Match(const std::vector<Descriptor>& a, const std::vector<Descriptor>& b,
                      const std::vector<bool>& maskA, const std::vector<bool>& maskB, int maxHammingDist,
                      int minHammingDifference, std::vector<DMatch>& goodMatches)
{
    std::vector<uint8_t> ma(maskA.begin(), maskA.end()), mb(maskB.begin(), maskB.end());
    goodMatches.resize(a.size());
    uint32_t n = 0;
    check(mage_hamming_match(a.empty() ? nullptr : a.front().data(), (uint32_t)a.size(), ma.empty() ? nullptr : ma.data(),
                             b.empty() ? nullptr : b.front().data(), (uint32_t)b.size(), mb.empty() ? nullptr : mb.data(),
                             maxHammingDist, minHammingDifference, goodMatches.data(), (uint32_t)goodMatches.size(), &n));
    goodMatches.resize(n);
    return n;
}

// RadiusMatch (FeatureMatcher.cpp:294-378): the target KeypointSpatialIndex is built on the device
// from targetKeypoints, so callers pass the keypoints instead of the index.  Optional position
// overrides and masks (nullptr = none).  Clears and fills goodMatches (query order).
inline unsigned RadiusMatch(const std::vector<KeyPoint>& queryKeypoints, const std::vector<float>* queryPositionOverrides,
                            const std::vector<bool>* queryKeypointsMask, const std::vector<Descriptor>& queryDescriptors,
                            const std::vector<KeyPoint>& targetKeypoints, const std::vector<bool>* targetKeypointsMask,
                            const std::vector<Descriptor>& targetDescriptors, float radius, int maxHammingDist,
                            int minHammingDifference, std::vector<DMatch>& goodMatches)
{
    std::vector<uint8_t> qm, tm;
    if (queryKeypointsMask) qm.assign(queryKeypointsMask->begin(), queryKeypointsMask->end());
    if (targetKeypointsMask) tm.assign(targetKeypointsMask->begin(), targetKeypointsMask->end());
    goodMatches.resize(queryKeypoints.size());
    uint32_t n = 0;
    check(mage_radius_match(queryKeypoints.data(), queryPositionOverrides ? queryPositionOverrides->data() : nullptr,
                            queryKeypointsMask ? qm.data() : nullptr,
                            queryDescriptors.empty() ? nullptr : queryDescriptors.front().data(), (uint32_t)queryKeypoints.size(),
                            targetKeypoints.data(), targetKeypointsMask ? tm.data() : nullptr,
                            targetDescriptors.empty() ? nullptr : targetDescriptors.front().data(),
                            (uint32_t)targetKeypoints.size(), radius, maxHammingDist, minHammingDifference,
                            goodMatches.data(), (uint32_t)goodMatches.size(), &n));
    goodMatches.resize(n);
    return n;
}

// TrackLocalMap's per-map-point matching loop (TrackLocalMap.cpp:175-256): projected map points in
// order (positions x, y interleaved; octaves; descriptors; the keypoint to hide for a
// pose-estimation outlier point, -1 otherwise) against a frame's keypoints; unassociatedMask is
// updated like the reference's (a match takes its keypoint).  Returns the keypoint per point or -1.
inline std::vector<int32_t> LocalMapMatch(const std::vector<float>& positions, const std::vector<int32_t>& octaves,
                                          const std::vector<Descriptor>& descriptors, const std::vector<int32_t>& hidden,
                                          const std::vector<KeyPoint>& targetKeypoints,
                                          const std::vector<Descriptor>& targetDescriptors,
                                          std::vector<bool>& unassociatedMask, float radius, int maxHammingDist,
                                          int minHammingDifference, int device = 0)
{
    const uint32_t n = (uint32_t)octaves.size();
    std::vector<uint8_t> mask(unassociatedMask.begin(), unassociatedMask.end());
    std::vector<int32_t> result(n, -1);
    check(mage_local_map_match(positions.data(), octaves.data(), descriptors.empty() ? nullptr : descriptors.front().data(),
                               hidden.empty() ? nullptr : hidden.data(), n, targetKeypoints.data(),
                               targetDescriptors.empty() ? nullptr : targetDescriptors.front().data(),
                               (uint32_t)targetKeypoints.size(), mask.data(), radius, maxHammingDist,
                               minHammingDifference, result.data(), device));
    for (size_t t = 0; t < mask.size(); t++) unassociatedMask[t] = mask[t] != 0;
    return result;
}

// OnlineBow vocabulary tree on the device (OnlineBow.cpp:289-311 FindLeafNode; nodes as CreateTree
// builds them: node i's descriptor, children in childrenIDs order, root 0).
class OnlineBowTree {
public:
    OnlineBowTree(const std::vector<Descriptor>& nodes, const std::vector<uint32_t>& childStart,
                  const std::vector<uint32_t>& children, int device = 0)
    {
        check(mage_bow_create(nodes.empty() ? nullptr : nodes.front().data(), childStart.data(),
                              children.empty() ? nullptr : children.data(), (uint32_t)nodes.size(), device, &m_handle));
    }
    // OnlineBow::CreateTree (OnlineBow.cpp:325-337) over training descriptors on the GPU
    // (BagOfWordsSettings TrainingTreeLevels / TrainingTreeBranchingFactor / MaxTrainingIteration)
    explicit OnlineBowTree(const std::vector<Descriptor>& training, unsigned levels = 2, unsigned branching = 6,
                           unsigned maxIterations = 12, int device = 0)
    {
        check(mage_bow_train(training.empty() ? nullptr : training.front().data(), (uint32_t)training.size(), levels,
                             branching, maxIterations, device, &m_handle));
    }
    ~OnlineBowTree() { mage_bow_destroy(m_handle); }
    OnlineBowTree(const OnlineBowTree&) = delete;
    OnlineBowTree& operator=(const OnlineBowTree&) = delete;
    ptrdiff_t FindLeafNode(const Descriptor& d) const
    {
        uint32_t leaf = 0;
        check(mage_bow_find_leaves(m_handle, d.data(), 1, &leaf));
        return (ptrdiff_t)leaf;
    }
    mage_bow* handle() const { return m_handle; }

private:
    mage_bow* m_handle = nullptr;
};

// IndexedMatch (FeatureMatcher.cpp:192-292) with the BoW candidate lists of `tree` (what
// OnlineBowFeatureMatcher / OnlineBow::QueryFeatures return); masks as in Match.
inline unsigned IndexedMatch(const OnlineBowTree& tree, const std::vector<Descriptor>& a, const std::vector<Descriptor>& b,
                             const std::vector<bool>& maskA, const std::vector<bool>& maskB, int maxHammingDist,
                             int minHammingDifference, std::vector<DMatch>& goodMatches)
{
    std::vector<uint8_t> ma(maskA.begin(), maskA.end()), mb(maskB.begin(), maskB.end());
    goodMatches.resize(a.size());
    uint32_t n = 0;
    check(mage_indexed_match(tree.handle(), a.empty() ? nullptr : a.front().data(), (uint32_t)a.size(),
                             ma.empty() ? nullptr : ma.data(), b.empty() ? nullptr : b.front().data(), (uint32_t)b.size(),
                             mb.empty() ? nullptr : mb.data(), maxHammingDist, minHammingDifference, goodMatches.data(),
                             (uint32_t)goodMatches.size(), &n));
    goodMatches.resize(n);
    return n;
}

// NewMapPointsCreationSettings (MageSettings.h:55-61) with CameraSettings' new-point grid
// (MageSettings.h:311-313) and the pyramid and image size of Ki.
struct NewMapPointsCreationSettings {
    float MinParallaxDegrees{0.0238961594253207f};
    float MaxEpipolarError{3.84385518580709f};
    float MinAcceptedDistanceRatio{2.0f};
    unsigned NewPointGridWidth{4}, NewPointGridHeight{3}, NewPointMaxGridCount{6};
    float PyramidScale{1.2f};
    unsigned NumLevels{8};
    unsigned ImageWidth{1280}, ImageHeight{720};
};

// What CreateInitialAssociations reads of a keyframe: Pose as view-space t and column-major R (the
// layout BundlerLib::SetCameraPose takes), the undistorted calibration {cx, cy, fx, fy}, the keypoints.
struct KeyframeView {
    std::array<float, 3> Position;
    std::array<float, 9> Rotation;
    std::array<float, 4> Intrinsics;
    const std::vector<KeyPoint>* KeyPoints;
};

using NewMapPoint = mage_new_point;

// CreateInitialAssociations' match loop (Mapping/NewMapPointsCreation.cpp:187-201, 277-321, with
// TryCreateNewAssociatedMapPointForMatch, :74-160): the matches of each covisible keyframe (in the
// order the reference visits them; queryIdx = Kc keypoint, trainIdx = Ki keypoint) against Ki.
// Returns the new points in the reference's push_back order; `verdicts`, when given, gets one
// MAGE_NP_* code per match and keyframe.  device < 0 runs the CPU backend.
inline std::vector<NewMapPoint> CreateInitialAssociations(const NewMapPointsCreationSettings& settings,
                                                          const KeyframeView& Ki,
                                                          const std::vector<bool>& KiAssociatedKeypointMask,
                                                          const std::vector<KeyframeView>& covisibleKeyframes,
                                                          const std::vector<std::vector<DMatch>>& matches,
                                                          std::vector<std::vector<uint8_t>>* verdicts = nullptr,
                                                          int device = 0)
{
    if (matches.size() != covisibleKeyframes.size())
        throw std::invalid_argument("one match list per covisible keyframe");
    mage_new_points_settings s{};
    s.struct_size = (uint32_t)sizeof(s);
    s.max_epipolar_error = settings.MaxEpipolarError;
    s.min_accepted_distance_ratio = settings.MinAcceptedDistanceRatio;
    s.min_parallax_degrees = settings.MinParallaxDegrees;
    s.pyramid_scale = settings.PyramidScale;
    s.num_levels = settings.NumLevels;
    s.grid_width = settings.NewPointGridWidth;
    s.grid_height = settings.NewPointGridHeight;
    s.max_grid_count = settings.NewPointMaxGridCount;
    s.image_width = settings.ImageWidth;
    s.image_height = settings.ImageHeight;
    const uint32_t n_kc = (uint32_t)covisibleKeyframes.size();
    std::vector<float> pos, rot, intr;
    std::vector<KeyPoint> kps;
    std::vector<DMatch> all;
    std::vector<uint32_t> kp_start(n_kc + 1, 0), m_start(n_kc + 1, 0);
    for (uint32_t k = 0; k < n_kc; k++) {
        const KeyframeView& kc = covisibleKeyframes[k];
        pos.insert(pos.end(), kc.Position.begin(), kc.Position.end());
        rot.insert(rot.end(), kc.Rotation.begin(), kc.Rotation.end());
        intr.insert(intr.end(), kc.Intrinsics.begin(), kc.Intrinsics.end());
        kps.insert(kps.end(), kc.KeyPoints->begin(), kc.KeyPoints->end());
        all.insert(all.end(), matches[k].begin(), matches[k].end());
        kp_start[k + 1] = (uint32_t)kps.size();
        m_start[k + 1] = (uint32_t)all.size();
    }
    std::vector<uint8_t> mask(KiAssociatedKeypointMask.begin(), KiAssociatedKeypointMask.end());
    if (!mask.empty() && mask.size() != Ki.KeyPoints->size())
        throw std::invalid_argument("KiAssociatedKeypointMask must have one entry per Ki keypoint");
    std::vector<NewMapPoint> out(std::max<size_t>(all.size(), 1));
    std::vector<uint8_t> verdict(std::max<size_t>(all.size(), 1), 0xFF);
    uint32_t n = 0, status = 0;
    const uint32_t n_ki = (uint32_t)Ki.KeyPoints->size();
    const uint8_t* pm = mask.empty() ? nullptr : mask.data();
    if (device < 0)
        check(mage_new_map_points_host(&s, Ki.Position.data(), Ki.Rotation.data(), Ki.Intrinsics.data(),
                                       Ki.KeyPoints->data(), n_ki, pm, n_kc, pos.data(), rot.data(), intr.data(),
                                       kps.data(), kp_start.data(), all.data(), m_start.data(), out.data(),
                                       (uint32_t)out.size(), &n, verdict.data(), &status));
    else
        check(mage_new_map_points(&s, Ki.Position.data(), Ki.Rotation.data(), Ki.Intrinsics.data(), Ki.KeyPoints->data(),
                                  n_ki, pm, n_kc, pos.data(), rot.data(), intr.data(), kps.data(), kp_start.data(),
                                  all.data(), m_start.data(), out.data(), (uint32_t)out.size(), &n, verdict.data(),
                                  &status, device));
    if (status & 1u) throw Error(MAGE_EUNSUPPORTED, "more than 4096 keypoints in Ki");
    out.resize(n);
    if (verdicts) {
        verdicts->assign(n_kc, {});
        for (uint32_t k = 0; k < n_kc; k++)
            (*verdicts)[k].assign(verdict.begin() + m_start[k], verdict.begin() + m_start[k + 1]);
    }
    return out;
}

// The association part of NewMapPointsCreationSettings (MageSettings.h:55-61) and Ki's image border.
struct NewPointsAssociationSettings {
    float NewMapPointsSearchRadius{11.8816156f};
    float MaxKeyframeAngleDegrees{60.0f};
    float KiImageBorder{0.0f};
    int MaxHammingDistance{30};  // AssociateMatcherSettings
    int MinHammingDifference{1};
};

// What LocallyAssociateNewAssociations reads of a covisible keyframe on top of KeyframeView: the
// descriptors, the unassociated-keypoint mask as IndexedMatch saw it (updated in place: the
// keypoints CreateInitialAssociations and this call associate become false) and the index the
// keyframe had among CreateInitialAssociations' covisibleKeyframes (its Kc slot), or -1.
struct MappingKeyframeView {
    KeyframeView View;
    const std::vector<Descriptor>* Descriptors;
    std::vector<bool>* UnassociatedKeypointMask;
    int Slot{-1};
};

struct KeyframeAssociation {
    int Keyframe;  // index into the covisible keyframes; -1 is Ki
    uint32_t Keypoint;
};

// MapPointKeyframeAssociations (NewMapPointsCreation.h): the new point and its Keyframes list,
// starting {Ki, Kc}.
struct MapPointKeyframeAssociations {
    NewMapPoint MapPoint;
    std::vector<KeyframeAssociation> Keyframes;
};

inline mage_new_points_settings ToC(const NewMapPointsCreationSettings& settings)
{
    mage_new_points_settings s{};
    s.struct_size = (uint32_t)sizeof(s);
    s.max_epipolar_error = settings.MaxEpipolarError;
    s.min_accepted_distance_ratio = settings.MinAcceptedDistanceRatio;
    s.min_parallax_degrees = settings.MinParallaxDegrees;
    s.pyramid_scale = settings.PyramidScale;
    s.num_levels = settings.NumLevels;
    s.grid_width = settings.NewPointGridWidth;
    s.grid_height = settings.NewPointGridHeight;
    s.max_grid_count = settings.NewPointMaxGridCount;
    s.image_width = settings.ImageWidth;
    s.image_height = settings.ImageHeight;
    return s;
}

// LocallyAssociateNewAssociations (Mapping/NewMapPointsCreation.cpp:337-424): every new point, in
// order, against every covisible keyframe (in the order CreateInitialAssociations' sort left) it is
// not yet associated with.  Returns per point the associations gained, in keyframe order; `verdicts`
// (points x keyframes, MAGE_NA_*) and `records` (projection, octave, keypoint) when given.
// device < 0 runs the CPU backend.
inline std::vector<std::vector<KeyframeAssociation>> LocallyAssociateNewAssociations(
    const NewMapPointsCreationSettings& settings, const NewPointsAssociationSettings& association,
    const std::vector<Descriptor>& KiDescriptors, const std::vector<MappingKeyframeView>& covisibleKeyframes,
    const std::vector<NewMapPoint>& newMapPoints, std::vector<uint8_t>* verdicts = nullptr,
    std::vector<mage_new_point_assoc>* records = nullptr, int device = 0)
{
    const mage_new_points_settings s = ToC(settings);
    mage_new_points_assoc_settings a{};
    a.struct_size = (uint32_t)sizeof(a);
    a.search_radius = association.NewMapPointsSearchRadius;
    a.max_keyframe_angle_degrees = association.MaxKeyframeAngleDegrees;
    a.image_border = association.KiImageBorder;
    a.max_hamming_distance = association.MaxHammingDistance;
    a.min_hamming_difference = association.MinHammingDifference;
    const uint32_t n_kf = (uint32_t)covisibleKeyframes.size(), n = (uint32_t)newMapPoints.size();
    std::vector<float> pos, rot, intr;
    std::vector<KeyPoint> kps;
    std::vector<uint8_t> desc, mask;
    std::vector<uint32_t> start(n_kf + 1, 0);
    std::vector<int32_t> slot(n_kf, -1);
    for (uint32_t k = 0; k < n_kf; k++) {
        const MappingKeyframeView& kf = covisibleKeyframes[k];
        const size_t nk = kf.View.KeyPoints->size();
        if (kf.Descriptors->size() != nk || kf.UnassociatedKeypointMask->size() != nk)
            throw std::invalid_argument("a keyframe's keypoints, descriptors and mask must have one length");
        pos.insert(pos.end(), kf.View.Position.begin(), kf.View.Position.end());
        rot.insert(rot.end(), kf.View.Rotation.begin(), kf.View.Rotation.end());
        intr.insert(intr.end(), kf.View.Intrinsics.begin(), kf.View.Intrinsics.end());
        kps.insert(kps.end(), kf.View.KeyPoints->begin(), kf.View.KeyPoints->end());
        for (const Descriptor& d : *kf.Descriptors) desc.insert(desc.end(), d.begin(), d.end());
        mask.insert(mask.end(), kf.UnassociatedKeypointMask->begin(), kf.UnassociatedKeypointMask->end());
        start[k + 1] = (uint32_t)kps.size();
        slot[k] = kf.Slot;
    }
    std::vector<mage_new_point_assoc> out(std::max<size_t>((size_t)n * n_kf, 1));
    std::vector<uint8_t> verdict(std::max<size_t>((size_t)n * n_kf, 1), 0xFF);
    uint32_t status = 0;
    const uint8_t* kid = KiDescriptors.empty() ? nullptr : KiDescriptors.front().data();
    if (device < 0)
        check(mage_new_points_associate_host(&s, &a, newMapPoints.data(), n, kid, (uint32_t)KiDescriptors.size(), n_kf,
                                             pos.data(), rot.data(), intr.data(), kps.data(), desc.data(), start.data(),
                                             slot.data(), mask.data(), out.data(), verdict.data(), &status));
    else
        check(mage_new_points_associate(&s, &a, newMapPoints.data(), n, kid, (uint32_t)KiDescriptors.size(), n_kf,
                                        pos.data(), rot.data(), intr.data(), kps.data(), desc.data(), start.data(),
                                        slot.data(), mask.data(), out.data(), verdict.data(), &status, device));
    if (status & 1u) throw Error(MAGE_EUNSUPPORTED, "more than 4096 keypoints in a covisible keyframe");
    std::vector<std::vector<KeyframeAssociation>> gained(n);
    for (uint32_t p = 0; p < n; p++)
        for (uint32_t k = 0; k < n_kf; k++)
            if (verdict[(size_t)p * n_kf + k] == MAGE_NA_ASSOCIATED)
                gained[p].push_back({(int)k, (uint32_t)out[(size_t)p * n_kf + k].keypoint});
    for (uint32_t k = 0; k < n_kf; k++)
        for (uint32_t t = start[k]; t < start[k + 1]; t++)
            (*covisibleKeyframes[k].UnassociatedKeypointMask)[t - start[k]] = mask[t] != 0;
    out.resize((size_t)n * n_kf);
    verdict.resize((size_t)n * n_kf);
    if (verdicts) *verdicts = verdict;
    if (records) *records = out;
    return gained;
}

// NewMapPointsCreation (Mapping/NewMapPointsCreation.cpp:426-446) after the reference's keyframe
// bookkeeping: `covisibleKeyframes` are all covisible keyframes in the order of :217, `matches[k]`
// the IndexedMatch(Kc, Ki) result of keyframe k — empty for a keyframe CreateInitialAssociations
// skipped or did not reach.  The keyframes with matches are the Kc slots, in order (at most 8).
// Returns every new point with its Keyframes list {Ki, Kc, gained...}; the keyframes' unassociated
// masks are updated.  device < 0 runs the CPU backend.
inline std::vector<MapPointKeyframeAssociations> NewMapPointsCreation(
    const NewMapPointsCreationSettings& settings, const NewPointsAssociationSettings& association, const KeyframeView& Ki,
    const std::vector<Descriptor>& KiDescriptors, const std::vector<bool>& KiAssociatedKeypointMask,
    std::vector<MappingKeyframeView>& covisibleKeyframes, const std::vector<std::vector<DMatch>>& matches, int device = 0)
{
    if (matches.size() != covisibleKeyframes.size())
        throw std::invalid_argument("one match list per covisible keyframe");
    std::vector<KeyframeView> kc;
    std::vector<std::vector<DMatch>> kcMatches;
    std::vector<int> kcOf;
    for (size_t k = 0; k < covisibleKeyframes.size(); k++) {
        covisibleKeyframes[k].Slot = -1;
        if (matches[k].empty()) continue;
        covisibleKeyframes[k].Slot = (int)kc.size();
        kc.push_back(covisibleKeyframes[k].View);
        kcMatches.push_back(matches[k]);
        kcOf.push_back((int)k);
    }
    const std::vector<NewMapPoint> points =
        CreateInitialAssociations(settings, Ki, KiAssociatedKeypointMask, kc, kcMatches, nullptr, device);
    const auto gained =
        LocallyAssociateNewAssociations(settings, association, KiDescriptors, covisibleKeyframes, points, nullptr, nullptr, device);
    std::vector<MapPointKeyframeAssociations> out(points.size());
    for (size_t p = 0; p < points.size(); p++) {
        out[p].MapPoint = points[p];
        out[p].Keyframes = {{-1, points[p].ki_index}, {kcOf[points[p].kc_slot], points[p].kc_index}};
        out[p].Keyframes.insert(out[p].Keyframes.end(), gained[p].begin(), gained[p].end());
    }
    return out;
}

// What the mapping task's cheap loop closure reads of the settings: LoopClosureSettings
// (MageSettings.h:197-207) with its CheapLoopClosureMatchingSettings, TrackLocalMapSettings' view
// angle and OrbMatcherSettings (:180-194), and the keyframes' image border, size and pyramid.
struct CheapLoopClosureSettings {
    unsigned MaxMapPoints{200}, MinKeyframe{10};
    float MatchSearchRadius{18.f};
    float MinDegreesBetweenCurrentViewAndMapPointView{60.f};
    float ImageBorder{7.5f};
    unsigned ImageWidth{640}, ImageHeight{480};
    unsigned NumLevels{1};
    float PyramidScale{1.5f};
    int CheapLoopClosureMaxHammingDistance{30}, CheapLoopClosureMinHammingDifference{1};
    int ConnectMaxHammingDistance{30}, ConnectMinHammingDifference{1};

    mage_loop_closure_settings ToC() const
    {
        mage_loop_closure_settings s{};
        s.struct_size = (uint32_t)sizeof(s);
        s.max_map_points = MaxMapPoints;
        s.min_keyframes = MinKeyframe;
        s.search_radius = MatchSearchRadius;
        s.min_view_degrees = MinDegreesBetweenCurrentViewAndMapPointView;
        s.image_border = ImageBorder;
        s.width = ImageWidth;
        s.height = ImageHeight;
        s.num_levels = NumLevels;
        s.pyramid_scale = PyramidScale;
        s.closure_max_hamming_distance = CheapLoopClosureMaxHammingDistance;
        s.closure_min_hamming_difference = CheapLoopClosureMinHammingDifference;
        s.connect_max_hamming_distance = ConnectMaxHammingDistance;
        s.connect_min_hamming_difference = ConnectMinHammingDifference;
        return s;
    }
};

using MapPointObservation = mage_map_point_obs;  // one entry of MapPoint::m_keyframes, as the refresh reads it
using MapPointState = mage_map_point_state;

// A map point as the step reads it: its derived state and its observations in m_keyframes' order.
struct MapPointView {
    MapPointState State{};
    std::vector<MapPointObservation> Observations;
};

// MapPoint::UpdateRepresentativeDescriptor and UpdateMeanViewDirectionAndDistances (Map/MapPoint.cpp:
// 80-155) for a point at `position` with the given observations.  device < 0 runs the CPU backend.
inline MapPointState UpdateMapPoint(const CheapLoopClosureSettings& settings, const std::array<float, 3>& position,
                                    const std::vector<MapPointObservation>& observations, int device = 0)
{
    const mage_loop_closure_settings s = settings.ToC();
    const uint32_t n = (uint32_t)observations.size();
    const MapPointObservation none{};
    MapPointState state{};
    const MapPointObservation* obs = n ? observations.data() : &none;
    if (device < 0)
        check(mage_map_points_refresh_host(&s, 1, position.data(), obs, std::max(n, 1u), &n, &state));
    else
        check(mage_map_points_refresh(&s, 1, position.data(), obs, std::max(n, 1u), &n, &state, device));
    return state;
}

// What the step reads of a keyframe on top of KeyframeView: its id, the descriptors, and per keypoint
// the index of the map point it is associated with, or -1 (HasMapPoint / IsAssociatedToMapPoint and,
// for the new keyframe, the unassociated mask).  UnassociatedKeypointMask (covisible keyframes;
// CreateUnassociatedMask) is updated in place.
struct LoopClosureKeyframe {
    int Id{0};
    KeyframeView View;
    const std::vector<Descriptor>* Descriptors{nullptr};
    const std::vector<int32_t>* KeypointMapPoints{nullptr};
    std::vector<bool>* UnassociatedKeypointMask{nullptr};
};

struct LoopClosureAssociation {
    uint32_t MapPoint;  // index into the map
    uint32_t Keypoint;
};

struct CheapLoopClosureResult {
    std::vector<LoopClosureAssociation> Associations;             // CheapLoopClosure's return value
    std::vector<std::vector<LoopClosureAssociation>> Connected;   // per covisible keyframe, TryConnectMapPoints' extraAssociations
    std::vector<bool> Modified;                                   // modifiedKeyframes: UpdateGraph is the caller's
    std::vector<uint32_t> Sample;                                 // GetSampleOfMapPoints, as map indices
    std::vector<mage_loop_closure_assoc> ClosureRecords, ConnectRecords;  // by place in the sample (x n_kf)
    std::vector<uint8_t> ClosureVerdicts, ConnectVerdicts;        // MAGE_LC_*
};

// MappingWorker.cpp:160-181: CheapLoopClosure (:20-73) of the map's sample into the new keyframe Ki,
// InsertKeyframe's associations (ThreadSafeMap.cpp:242-249) and TryConnectMapPoints (:715-787) over
// the covisible keyframes in the given order.  The associated map points gain their observations and
// are refreshed in `map`; the covisible keyframes' masks are updated.  `loopCounter` is the mapping
// task's frame counter, `keyframeCount` the map's GetKeyframesCount().  device < 0 runs the CPU
// backend.  Throws Error (MAGE_EUNSUPPORTED) for a keyframe with more than 4096 keypoints.
inline CheapLoopClosureResult CheapLoopClosureAndConnect(const CheapLoopClosureSettings& settings,
                                                         std::vector<MapPointView>& map, uint32_t loopCounter,
                                                         uint32_t keyframeCount, const LoopClosureKeyframe& Ki,
                                                         const std::vector<LoopClosureKeyframe>& covisibleKeyframes,
                                                         int device = 0)
{
    const mage_loop_closure_settings s = settings.ToC();
    const uint32_t n_kf = (uint32_t)covisibleKeyframes.size(), n_map = (uint32_t)map.size(), max = settings.MaxMapPoints;
    size_t pitch = 0;
    for (const MapPointView& p : map) {
        if ((size_t)p.State.n_obs != p.Observations.size()) throw std::invalid_argument("State.n_obs must count the observations");
        pitch = std::max(pitch, p.Observations.size());
    }
    pitch += 1 + (size_t)n_kf;  // room for every association the step can make
    std::vector<MapPointState> state(n_map);
    std::vector<MapPointObservation> obs((size_t)n_map * pitch);
    for (uint32_t i = 0; i < n_map; i++) {
        state[i] = map[i].State;
        std::copy(map[i].Observations.begin(), map[i].Observations.end(), obs.begin() + (size_t)i * pitch);
    }
    auto lengths = [](const LoopClosureKeyframe& kf) {
        const size_t nk = kf.View.KeyPoints->size();
        if (!kf.Descriptors || !kf.KeypointMapPoints || kf.Descriptors->size() != nk || kf.KeypointMapPoints->size() != nk)
            throw std::invalid_argument("a keyframe's keypoints, descriptors and map points must have one length");
        return nk;
    };
    const size_t n_ki = lengths(Ki);
    std::vector<uint8_t> ki_desc;
    for (const Descriptor& d : *Ki.Descriptors) ki_desc.insert(ki_desc.end(), d.begin(), d.end());
    std::vector<float> pos, rot, intr;
    std::vector<KeyPoint> kps;
    std::vector<uint8_t> desc, mask;
    std::vector<int32_t> point, ids(n_kf);
    std::vector<uint32_t> start(n_kf + 1, 0);
    for (uint32_t k = 0; k < n_kf; k++) {
        const LoopClosureKeyframe& kf = covisibleKeyframes[k];
        if (!kf.UnassociatedKeypointMask || kf.UnassociatedKeypointMask->size() != lengths(kf))
            throw std::invalid_argument("a covisible keyframe needs its unassociated mask");
        pos.insert(pos.end(), kf.View.Position.begin(), kf.View.Position.end());
        rot.insert(rot.end(), kf.View.Rotation.begin(), kf.View.Rotation.end());
        intr.insert(intr.end(), kf.View.Intrinsics.begin(), kf.View.Intrinsics.end());
        kps.insert(kps.end(), kf.View.KeyPoints->begin(), kf.View.KeyPoints->end());
        for (const Descriptor& d : *kf.Descriptors) desc.insert(desc.end(), d.begin(), d.end());
        point.insert(point.end(), kf.KeypointMapPoints->begin(), kf.KeypointMapPoints->end());
        mask.insert(mask.end(), kf.UnassociatedKeypointMask->begin(), kf.UnassociatedKeypointMask->end());
        start[k + 1] = (uint32_t)kps.size();
        ids[k] = kf.Id;
    }
    CheapLoopClosureResult r;
    r.Sample.resize(max);
    r.ClosureRecords.resize(max);
    r.ClosureVerdicts.assign(max, 0xFF);
    r.ConnectRecords.resize(std::max<size_t>((size_t)max * n_kf, 1));
    r.ConnectVerdicts.assign(std::max<size_t>((size_t)max * n_kf, 1), 0xFF);
    std::vector<uint8_t> ki_mask(std::max<size_t>(n_ki, 1)), modified(std::max<uint32_t>(n_kf, 1));
    uint32_t counts[3] = {0, 0, 0}, status = 0;
    mage_loop_closure_problem p{};
    p.struct_size = (uint32_t)sizeof(p);
    p.n_map = n_map;
    p.state = state.data();
    p.obs = obs.data();
    p.obs_pitch = (int64_t)pitch;
    p.offset = loopCounter;
    p.n_keyframes = keyframeCount;
    p.ki_id = Ki.Id;
    p.n_ki = (uint32_t)n_ki;
    p.ki_pos3 = Ki.View.Position.data();
    p.ki_r9 = Ki.View.Rotation.data();
    p.ki_intr4 = Ki.View.Intrinsics.data();
    p.ki_kp = Ki.View.KeyPoints->data();
    p.ki_desc = ki_desc.data();
    p.ki_point = Ki.KeypointMapPoints->data();
    p.n_kf = n_kf;
    p.kf_id = ids.data();
    p.kf_pos3 = pos.data();
    p.kf_r9 = rot.data();
    p.kf_intr4 = intr.data();
    p.kf_kp = kps.data();
    p.kf_desc = desc.data();
    p.kf_point = point.data();
    p.kf_start = start.data();
    p.kf_mask = mask.data();
    p.sample_index = r.Sample.data();
    p.closure = r.ClosureRecords.data();
    p.closure_verdict = r.ClosureVerdicts.data();
    p.connect = r.ConnectRecords.data();
    p.connect_verdict = r.ConnectVerdicts.data();
    p.ki_mask = ki_mask.data();
    p.kf_modified = modified.data();
    p.counts = counts;
    p.status = &status;
    check(device < 0 ? mage_cheap_loop_closure_host(&s, &p) : mage_cheap_loop_closure(&s, &p, device));
    if (status & MAGE_LC_STATUS_OVER_LIMIT) throw Error(MAGE_EUNSUPPORTED, "more than 4096 keypoints in a keyframe");
    const uint32_t L = counts[0];
    r.Sample.resize(L);
    r.ClosureRecords.resize(L);
    r.ClosureVerdicts.resize(L);
    r.ConnectRecords.resize((size_t)L * n_kf);
    r.ConnectVerdicts.resize((size_t)L * n_kf);
    r.Connected.assign(n_kf, {});
    r.Modified.assign(n_kf, false);
    for (uint32_t j = 0; j < L; j++) {
        const uint32_t i = r.Sample[j];
        if (r.ClosureRecords[j].keypoint >= 0) r.Associations.push_back({i, (uint32_t)r.ClosureRecords[j].keypoint});
        for (uint32_t k = 0; k < n_kf; k++)
            if (r.ConnectRecords[(size_t)j * n_kf + k].keypoint >= 0)
                r.Connected[k].push_back({i, (uint32_t)r.ConnectRecords[(size_t)j * n_kf + k].keypoint});
        map[i].State = state[i];
        map[i].Observations.assign(obs.begin() + (size_t)i * pitch, obs.begin() + (size_t)i * pitch + state[i].n_obs);
    }
    if (L)
        for (uint32_t k = 0; k < n_kf; k++) {
            r.Modified[k] = modified[k] != 0;
            for (uint32_t t = start[k]; t < start[k + 1]; t++)
                (*covisibleKeyframes[k].UnassociatedKeypointMask)[t - start[k]] = mask[t] != 0;
        }
    return r;
}

// CheapLoopClosure (MappingWorker.cpp:20-73) with InsertKeyframe's associations alone.
inline CheapLoopClosureResult CheapLoopClosure(const CheapLoopClosureSettings& settings, std::vector<MapPointView>& map,
                                               uint32_t loopCounter, uint32_t keyframeCount, const LoopClosureKeyframe& Ki,
                                               int device = 0)
{
    return CheapLoopClosureAndConnect(settings, map, loopCounter, keyframeCount, Ki, {}, device);
}

// StereoMapInitializationSettings (MageSettings.h:135-147) with its OrbMatcherSettings and
// BundleAdjustSettings bags (:36-52).
struct StereoMapInitializationSettings {
    unsigned MinInitMapPoints{15}, MinFeatureMatches{40};
    float MaxOutlierError{2.5f};
    float MaxEpipolarError{5.5f};
    float MinAcceptedDistanceRatio{2.0f};
    float InitializationTetherStrength{50.0f};
    float MaxPoseContributionZ{0.10f};
    float AmountBACanChangePose{1.65f};
    float MaxDepthMeters{2.3f};
    struct {
        int MaxHammingDistance{30}, MinHammingDifference{1};
    } OrbMatcherSettings;
    struct {
        unsigned NumSteps{1}, NumStepsPerRun{1}, MinSteps{1};
        float HuberWidth{1.8f}, HuberWidthScale{0.95f}, MaxOutlierError{7.25f}, MaxOutlierErrorScaleFactor{0.95f};
        float MinMeanSquareError{0.25f}, DistanceTetherWeight{50.f}, LowConnectivityIterationsScale{1.5f};
    } BundleAdjustSettings;

    mage_stereo_init_settings ToC() const
    {
        mage_stereo_init_settings s{};
        s.struct_size = (uint32_t)sizeof(s);
        s.min_init_map_points = MinInitMapPoints;
        s.min_feature_matches = MinFeatureMatches;
        s.max_outlier_error = MaxOutlierError;
        s.max_epipolar_error = MaxEpipolarError;
        s.min_accepted_distance_ratio = MinAcceptedDistanceRatio;
        s.initialization_tether_strength = InitializationTetherStrength;
        s.max_pose_contribution_z = MaxPoseContributionZ;
        s.amount_ba_can_change_pose = AmountBACanChangePose;
        s.max_depth_meters = MaxDepthMeters;
        s.max_hamming_distance = OrbMatcherSettings.MaxHammingDistance;
        s.min_hamming_difference = OrbMatcherSettings.MinHammingDifference;
        s.ba_num_steps = BundleAdjustSettings.NumSteps;
        s.ba_num_steps_per_run = BundleAdjustSettings.NumStepsPerRun;
        s.ba_min_steps = BundleAdjustSettings.MinSteps;
        s.ba_huber_width = BundleAdjustSettings.HuberWidth;
        s.ba_huber_width_scale = BundleAdjustSettings.HuberWidthScale;
        s.ba_max_outlier_error = BundleAdjustSettings.MaxOutlierError;
        s.ba_max_outlier_error_scale_factor = BundleAdjustSettings.MaxOutlierErrorScaleFactor;
        s.ba_min_mean_square_error = BundleAdjustSettings.MinMeanSquareError;
        s.ba_distance_tether_weight = BundleAdjustSettings.DistanceTetherWeight;
        s.ba_low_connectivity_iterations_scale = BundleAdjustSettings.LowConnectivityIterationsScale;
        return s;
    }
};

using StereoPoint = mage_stereo_point;

// What StereoMapInit::Initialize has when InitializeWithFrames returns (StereoMapInit.cpp:47-88,
// :104-159): frame 0's crop mask, Match's result, one MAGE_ST_* verdict per match, the accepted
// matches with their points in match order (the two keyframe builders' associations are QueryIdx
// in frame 0 and TrainIdx in frame 1, :83-87) and the arrays BundleAdjustInitializationData gives
// the bundler (BundlerLib::SetMapPoint / SetObservation order).
struct StereoTriangulation {
    std::vector<bool> Frame0Mask;
    std::vector<DMatch> Matches;
    std::vector<uint8_t> Verdicts;
    std::vector<StereoPoint> Points;
    std::vector<float> BundlePoints, BundleObservations, BundleInformation;
    std::vector<uint32_t> BundleCameras, BundleMapPoints;
};

// The stretch of StereoMapInit::Initialize between the crop (:100) and the map-point count test
// (:161) for one pair: frame 0's keypoints masked to `crop` {x, y, width, height}, the masked frame 0
// matched against frame 1, every match through MapInitialization::TriangulatePoints with frame 0
// as the reference frame.  Descriptors are n x 32 bytes per frame; with `matches` given they are not
// read and no matcher runs.  device < 0 runs the CPU backend, which needs `matches`.
inline StereoTriangulation TriangulateStereoPair(const StereoMapInitializationSettings& settings,
                                                 const KeyframeView& frame0, const uint8_t* frame0Descriptors,
                                                 const KeyframeView& frame1, const uint8_t* frame1Descriptors,
                                                 const std::array<int32_t, 4>& crop,
                                                 const std::vector<DMatch>* matches = nullptr, int device = 0)
{
    if (!matches && (device < 0 || !frame0Descriptors || !frame1Descriptors))
        throw std::invalid_argument("without matches both descriptor sets and a device are needed");
    const mage_stereo_init_settings s = settings.ToC();
    const uint32_t n0 = (uint32_t)frame0.KeyPoints->size(), n1 = (uint32_t)frame1.KeyPoints->size();
    float pos[6], rot[18], intr[8];
    for (int f = 0; f < 2; f++) {
        const KeyframeView& v = f ? frame1 : frame0;
        std::copy(v.Position.begin(), v.Position.end(), pos + 3 * f);
        std::copy(v.Rotation.begin(), v.Rotation.end(), rot + 9 * f);
        std::copy(v.Intrinsics.begin(), v.Intrinsics.end(), intr + 4 * f);
    }
    StereoTriangulation r;
    if (matches) r.Matches = *matches;
    uint32_t nm = (uint32_t)r.Matches.size();
    const uint32_t cap = std::max<uint32_t>(matches ? nm : n0, 1);
    r.Matches.resize(cap);
    std::vector<uint8_t> mask(std::max<uint32_t>(n0, 1));
    r.Verdicts.assign(cap, 0xFF);
    r.Points.resize(cap);
    r.BundlePoints.resize(3 * (size_t)cap);
    r.BundleObservations.resize(4 * (size_t)cap);
    r.BundleInformation.resize(2 * (size_t)cap);
    r.BundleCameras.resize(2 * (size_t)cap);
    r.BundleMapPoints.resize(2 * (size_t)cap);
    uint32_t masked = 0, n = 0, status = 0;
    if (device < 0)
        check(mage_stereo_init_triangulate_host(&s, pos, rot, intr, crop.data(), frame0.KeyPoints->data(), n0,
                                                frame1.KeyPoints->data(), n1, r.Matches.data(), nm, mask.data(), &masked,
                                                r.Verdicts.data(), r.Points.data(), cap, &n, r.BundlePoints.data(),
                                                r.BundleObservations.data(), r.BundleCameras.data(),
                                                r.BundleMapPoints.data(), r.BundleInformation.data(), &status));
    else
        check(mage_stereo_init_triangulate(&s, pos, rot, intr, crop.data(), frame0.KeyPoints->data(),
                                           matches ? nullptr : frame0Descriptors, n0, frame1.KeyPoints->data(),
                                           matches ? nullptr : frame1Descriptors, n1, r.Matches.data(), cap, &nm,
                                           mask.data(), &masked, r.Verdicts.data(), r.Points.data(), cap, &n,
                                           r.BundlePoints.data(), r.BundleObservations.data(), r.BundleCameras.data(),
                                           r.BundleMapPoints.data(), r.BundleInformation.data(), &status, device));
    if (status & MAGE_ST_STATUS_OVER_LIMIT) throw Error(MAGE_EUNSUPPORTED, "more than 4096 keypoints in a frame");
    r.Frame0Mask.assign(mask.begin(), mask.begin() + n0);
    r.Matches.resize(nm);
    r.Verdicts.resize(nm);
    r.Points.resize(n);
    r.BundlePoints.resize(3 * (size_t)n);
    r.BundleObservations.resize(4 * (size_t)n);
    r.BundleInformation.resize(2 * (size_t)n);
    r.BundleCameras.resize(2 * (size_t)n);
    r.BundleMapPoints.resize(2 * (size_t)n);
    return r;
}

// What StereoMapInit::Initialize reads of an AnalyzedImage: the undistorted calibration and size
// (the extrinsics field is not read), the keypoints and their 32-byte descriptors.
struct StereoFrame {
    mage_camera_config Camera;
    const std::vector<KeyPoint>* KeyPoints;
    const uint8_t* Descriptors;
};

// The reference's InitializationData for a stereo pair: two keyframe builders — frame 0 at the
// identity, frame 1 at Frame1Position / Frame1Rotation (view-space t, column-major R) — and the
// map points; MapPoints[i] is associated with keypoint query_idx of frame 0 and train_idx of frame 1.
struct InitializationData {
    std::array<float, 3> Frame1Position;
    std::array<float, 9> Frame1Rotation;
    std::vector<StereoPoint> MapPoints;
};

// StereoMapInit (Stereo/StereoMapInit.h:23-35) over mage_stereo_map_init.
class StereoMapInit {
public:
    explicit StereoMapInit(const StereoMapInitializationSettings& settings, int device = 0)
        : m_settings(settings.ToC()), m_device(device)
    {
    }

    // Initialize (Stereo/StereoMapInit.cpp:97-194): std::nullopt where the reference returns
    // boost::none; LastResult() then says why (MAGE_STEREO_INIT_*).
    std::optional<InitializationData> Initialize(const StereoFrame& frame0, const StereoFrame& frame1,
                                                 const std::array<float, 16>& frame0ToFrame1)
    {
        const uint32_t n0 = (uint32_t)frame0.KeyPoints->size(), n1 = (uint32_t)frame1.KeyPoints->size();
        const size_t cap = std::max<size_t>(n0, 1);
        const size_t runs = m_settings.ba_num_steps / std::max(m_settings.ba_num_steps_per_run, 1u) + 2;
        std::vector<uint8_t> mask(cap), verdict(cap);
        std::vector<DMatch> matches(cap);
        std::vector<StereoPoint> points(cap);
        std::vector<uint32_t> outliers(2 * cap * runs);
        m_last = mage_stereo_map_init_result{};
        check(mage_stereo_map_init(&m_settings, frame0ToFrame1.data(), &frame0.Camera, &frame1.Camera,
                                   frame0.KeyPoints->data(), frame0.Descriptors, n0, frame1.KeyPoints->data(),
                                   frame1.Descriptors, n1, &m_last, mask.data(), matches.data(), verdict.data(),
                                   points.data(), outliers.data(), m_device));
        if (m_last.code != MAGE_STEREO_INIT_OK) return std::nullopt;
        InitializationData d;
        std::copy(m_last.frame1_pos3, m_last.frame1_pos3 + 3, d.Frame1Position.begin());
        std::copy(m_last.frame1_r9, m_last.frame1_r9 + 9, d.Frame1Rotation.begin());
        d.MapPoints.assign(points.begin(), points.begin() + m_last.n_points);
        return d;
    }

    const mage_stereo_map_init_result& LastResult() const { return m_last; }

private:
    mage_stereo_init_settings m_settings;
    int m_device;
    mage_stereo_map_init_result m_last{};
};

// MonoMapInitializationSettings (MageSettings.h:95-128) with its two OrbMatcherSettings bags.
struct MonoMapInitializationSettings {
    float FundamentalTransferErrorThreshold{1.1f};
    unsigned MinFeatureMatches{65}, MinScoringInliers{50};
    float MinInlierPercentage{0.5f};
    unsigned MinInitialMapPoints{40}, MinMapPoints{60};
    float MinThirdFrameMatchPercentage{0.5f}, FeatureCovisibilityThreshold{0.35f};
    float MaxParallax3dDistance{500.0f}, MaxParallax3dMedianDistance{20.0f};
    float MinCandidatePoseDisimilarity{0.3f}, MaxPoseContributionZ{0.66f};
    unsigned BundleAdjustmentG2OSteps{5};
    float BundleAdjustmentHuberWidth{1.5f};
    unsigned RansacIterationsForModels{90};
    float MaxEpipolarError{3.5f}, MaxOutlierError{2.5f}, AmountBACanChangePose{1.65f};
    float MapInitializationNewPointsCreationMinDistance{0.25f};
    unsigned MapInitFrameIntervalMilliseconds{0}, MinInitializationIntervalMilliseconds{150};
    unsigned MaxInitializationIntervalMilliseconds{540};
    float MinPixelSpread{40.0f};
    float FinalBA_HuberWidth{0.9f}, FinalBA_MaxOutlierError{4.0f}, FinalBA_MaxOutlierErrorScaleFactor{0.75f};
    float FinalBA_MinMeanSquareError{0.0f};
    unsigned FinalBA_NumStepsPerRun{5}, FinalBA_NumSteps{15};
    float ExtraFrame_MaxOutlierError{8.0f};
    unsigned ExtraFrame_BundleAdjustmentSteps{5};
    float ExtraFrame_HuberWidth{4.0f}, ExtraFrame_SearchRadius{40.0f};
    struct {
        int MaxHammingDistance{30}, MinHammingDifference{1};
    } FivePointMatchingSettings, ExtraFrameMatchingSettings;

    mage_mono_init_settings ToC() const
    {
        mage_mono_init_settings s{};
        s.struct_size = (uint32_t)sizeof(s);
        s.fundamental_transfer_error_threshold = FundamentalTransferErrorThreshold;
        s.min_feature_matches = MinFeatureMatches;
        s.min_scoring_inliers = MinScoringInliers;
        s.min_inlier_percentage = MinInlierPercentage;
        s.min_initial_map_points = MinInitialMapPoints;
        s.min_map_points = MinMapPoints;
        s.min_third_frame_match_percentage = MinThirdFrameMatchPercentage;
        s.feature_covisibility_threshold = FeatureCovisibilityThreshold;
        s.max_parallax_3d_distance = MaxParallax3dDistance;
        s.max_parallax_3d_median_distance = MaxParallax3dMedianDistance;
        s.min_candidate_pose_disimilarity = MinCandidatePoseDisimilarity;
        s.max_pose_contribution_z = MaxPoseContributionZ;
        s.bundle_adjustment_g2o_steps = BundleAdjustmentG2OSteps;
        s.bundle_adjustment_huber_width = BundleAdjustmentHuberWidth;
        s.ransac_iterations_for_models = RansacIterationsForModels;
        s.max_epipolar_error = MaxEpipolarError;
        s.max_outlier_error = MaxOutlierError;
        s.amount_ba_can_change_pose = AmountBACanChangePose;
        s.map_initialization_new_points_creation_min_distance = MapInitializationNewPointsCreationMinDistance;
        s.map_init_frame_interval_milliseconds = MapInitFrameIntervalMilliseconds;
        s.min_initialization_interval_milliseconds = MinInitializationIntervalMilliseconds;
        s.max_initialization_interval_milliseconds = MaxInitializationIntervalMilliseconds;
        s.min_pixel_spread = MinPixelSpread;
        s.final_ba_huber_width = FinalBA_HuberWidth;
        s.final_ba_max_outlier_error = FinalBA_MaxOutlierError;
        s.final_ba_max_outlier_error_scale_factor = FinalBA_MaxOutlierErrorScaleFactor;
        s.final_ba_min_mean_square_error = FinalBA_MinMeanSquareError;
        s.final_ba_num_steps_per_run = FinalBA_NumStepsPerRun;
        s.final_ba_num_steps = FinalBA_NumSteps;
        s.extra_frame_max_outlier_error = ExtraFrame_MaxOutlierError;
        s.extra_frame_bundle_adjustment_steps = ExtraFrame_BundleAdjustmentSteps;
        s.extra_frame_huber_width = ExtraFrame_HuberWidth;
        s.extra_frame_search_radius = ExtraFrame_SearchRadius;
        s.five_point_max_hamming_distance = FivePointMatchingSettings.MaxHammingDistance;
        s.five_point_min_hamming_difference = FivePointMatchingSettings.MinHammingDifference;
        s.extra_frame_max_hamming_distance = ExtraFrameMatchingSettings.MaxHammingDistance;
        s.extra_frame_min_hamming_difference = ExtraFrameMatchingSettings.MinHammingDifference;
        return s;
    }
};

// What MapInitialization::InitializeWithFrames reads of an AnalyzedImage: the undistorted
// calibration {cx, cy, fx, fy}, the undistorted keypoints and (for the matcher) their descriptors.
struct MonoFrame {
    std::array<float, 4> Intrinsics;
    const std::vector<KeyPoint>* KeyPoints;
    const uint8_t* Descriptors{nullptr};  // n x 32 bytes, or null when the matches are given
};

// The reference's InitializationData after InitializeWithFrames (MapInitialization.cpp:1030-1091):
// the reference frame's builder at the identity, the current frame's at Frame1Position /
// Frame1Rotation (view-space t, column-major R), and the map points in match order; MapPoints[i] is
// associated with keypoint query_idx of the reference frame and train_idx of the current frame.
// The Bundle* arrays are BundleAdjustInitializationData's inputs for these two frames.
struct MonoInitializationData {
    std::array<float, 3> Frame1Position;
    std::array<float, 9> Frame1Rotation;
    std::vector<StereoPoint> MapPoints;
    std::vector<float> BundlePoints, BundleObservations, BundleInformation;
    std::vector<uint32_t> BundleCameras, BundleMapPoints;
};

// The third frame as LocateThirdFrame leaves it.  The reference keeps the MIDPOINT pose for the frame
// (MapInitialization.cpp:840) and drops OptimizeCameraPose's result; both are here.
struct MonoThirdFrame {
    std::array<float, 3> Position, OptimizedPosition;  // view-space t
    std::array<float, 9> Rotation, OptimizedRotation;  // column-major R
    std::vector<int32_t> KeyPointOf;     // per map point: its keypoint in the third frame, or -1
    std::vector<uint8_t> Verdicts;       // per map point: MAGE_M3_PT_*
    std::vector<int32_t> Distances;      // per map point: best distance of frame 0's / frame 1's query, or -1
    std::vector<float> Projections;      // per map point: x, y through the midpoint pose
    std::vector<uint8_t> Unassociated;   // per third-frame keypoint: 1 = still free after the matching
    std::vector<float> Observations;     // the surviving associations as bundle-adjustment observations
    std::vector<uint32_t> ObservationPoints, ObservationCameras;
    std::vector<float> ObservationInformation;
    std::vector<uint8_t> Outliers;       // a device ran: the bundle adjustment's flag per matched point
};

// The two-view stage and the third frame of MapInitialization (Tracking/MapInitialization.h) over
// mage_mono_init_two_view and mage_mono_init_third_frame.
class MonoMapInit {
public:
    // device < 0 runs the CPU backend, which needs the matches.
    explicit MonoMapInit(const MonoMapInitializationSettings& settings, int device = 0)
        : m_settings(settings.ToC()), m_device(device)
    {
    }

    // InitializeWithFrames (MapInitialization.cpp:988-1094) for the caller's bestMatches (queryIdx in
    // the reference frame, trainIdx in the current frame); with `matches` null the octave-0 masks
    // and Match of :562-588 run first (a device and both descriptor sets are needed).  std::nullopt
    // where the reference returns false; LastResult().verdict then says why (MAGE_MI_*) and
    // LastMatches() holds the matches the stage ran on.  Throws where the reference asserts or would
    // read out of bounds: a match that names no keypoint (std::out_of_range), more than 4096
    // keypoints or matches (Error, MAGE_EUNSUPPORTED).
    std::optional<MonoInitializationData> InitializeWithFrames(const std::vector<DMatch>* matches,
                                                               const MonoFrame& referenceFrame,
                                                               const MonoFrame& currentFrame)
    {
        if (!matches && (m_device < 0 || !referenceFrame.Descriptors || !currentFrame.Descriptors))
            throw std::invalid_argument("without matches both descriptor sets and a device are needed");
        const uint32_t n0 = (uint32_t)referenceFrame.KeyPoints->size(), n1 = (uint32_t)currentFrame.KeyPoints->size();
        float intr[8];
        std::copy(referenceFrame.Intrinsics.begin(), referenceFrame.Intrinsics.end(), intr);
        std::copy(currentFrame.Intrinsics.begin(), currentFrame.Intrinsics.end(), intr + 4);
        m_matches = matches ? *matches : std::vector<DMatch>();
        uint32_t nm = (uint32_t)m_matches.size();
        const uint32_t cap = std::max<uint32_t>(matches ? nm : std::min<uint32_t>(n0, 4096u), 1);
        m_matches.resize(cap);
        MonoInitializationData d;
        d.MapPoints.resize(cap);
        d.BundlePoints.resize(3 * (size_t)cap);
        d.BundleObservations.resize(4 * (size_t)cap);
        d.BundleInformation.resize(2 * (size_t)cap);
        d.BundleCameras.resize(2 * (size_t)cap);
        d.BundleMapPoints.resize(2 * (size_t)cap);
        m_last = mage_mono_init_result{};
        if (m_device < 0)
            check(mage_mono_init_two_view_host(&m_settings, intr, referenceFrame.KeyPoints->data(), n0,
                                               currentFrame.KeyPoints->data(), n1, m_matches.data(), nm, &m_last,
                                               d.MapPoints.data(), cap, d.BundlePoints.data(),
                                               d.BundleObservations.data(), d.BundleCameras.data(),
                                               d.BundleMapPoints.data(), d.BundleInformation.data(), nullptr));
        else
            check(mage_mono_init_two_view(&m_settings, intr, referenceFrame.KeyPoints->data(),
                                          matches ? nullptr : referenceFrame.Descriptors, n0,
                                          currentFrame.KeyPoints->data(), matches ? nullptr : currentFrame.Descriptors,
                                          n1, m_matches.data(), cap, &nm, &m_last, d.MapPoints.data(), cap,
                                          d.BundlePoints.data(), d.BundleObservations.data(), d.BundleCameras.data(),
                                          d.BundleMapPoints.data(), d.BundleInformation.data(), nullptr, m_device));
        m_matches.resize(nm);
        if (m_last.status & MAGE_MI_STATUS_OVER_LIMIT)
            throw Error(MAGE_EUNSUPPORTED, "more than 4096 keypoints in a frame or more than 4096 matches");
        if (m_last.status & MAGE_MI_STATUS_BAD_INDEX) throw std::out_of_range("a match names no keypoint");
        if (m_last.verdict != MAGE_MI_OK) return std::nullopt;
        const size_t n = m_last.n_points;
        std::copy(m_last.pos3 + 3, m_last.pos3 + 6, d.Frame1Position.begin());
        std::copy(m_last.r9 + 9, m_last.r9 + 18, d.Frame1Rotation.begin());
        d.MapPoints.resize(n);
        d.BundlePoints.resize(3 * n);
        d.BundleObservations.resize(4 * n);
        d.BundleInformation.resize(2 * n);
        d.BundleCameras.resize(2 * n);
        d.BundleMapPoints.resize(2 * n);
        return d;
    }

    // The third frame of TryIntializeMapWithProvidedFrames (MapInitialization.cpp:695-840): the middle
    // frame at the midpoint pose of the pair, every map point (points: xyz in MapPoints order, with its
    // keypoint index in frame 0 and frame 1) looked up in it under both descriptor bags, the pose-only
    // bundle adjustment, the cull and the two gates.  std::nullopt where the reference returns false;
    // LastThirdResult().verdict then says why (MAGE_M3_*).  The CPU backend (device < 0) has no pose
    // bundle adjustment: it takes its outcome in `ba` (null stops it after the first gate, and a
    // frame that passed it is then returned as it stands).  Throws as InitializeWithFrames does.
    struct ThirdFrameBA {
        std::vector<uint8_t> Outlier;  // per matched point, in point order
        std::array<float, 3> Position;
        std::array<float, 9> Rotation;
        float MeanSquareError;
    };
    std::optional<MonoThirdFrame> LocateThirdFrame(const std::array<float, 6>& positions,
                                                   const std::array<float, 18>& rotations,
                                                   const std::vector<float>& points,
                                                   const std::vector<int32_t>& frame0Index,
                                                   const std::vector<int32_t>& frame1Index, const uint8_t* descriptors0,
                                                   uint32_t n0, const uint8_t* descriptors1, uint32_t n1,
                                                   const MonoFrame& thirdFrame, uint32_t cameraIndex,
                                                   const ThirdFrameBA* ba = nullptr)
    {
        const uint32_t n = (uint32_t)frame0Index.size();
        if (points.size() != 3 * (size_t)n || frame1Index.size() != n)
            throw std::invalid_argument("one position and two keypoint indices per map point");
        if (!thirdFrame.Descriptors && !thirdFrame.KeyPoints->empty())
            throw std::invalid_argument("the third frame's descriptors are needed");
        const uint32_t n2 = (uint32_t)thirdFrame.KeyPoints->size();
        MonoThirdFrame f;
        f.KeyPointOf.resize(n);
        f.Verdicts.resize(n);
        f.Distances.resize(2 * (size_t)n);
        f.Projections.resize(2 * (size_t)n);
        f.Unassociated.resize(n2);
        f.Observations.resize(2 * (size_t)n);
        f.ObservationPoints.resize(n);
        f.ObservationCameras.resize(n);
        f.ObservationInformation.resize(n);
        f.Outliers.resize(n);
        m_third = mage_mono_init_third_result{};
        if (m_device < 0)
            check(mage_mono_init_third_frame_host(
                &m_settings, thirdFrame.Intrinsics.data(), positions.data(), rotations.data(), points.data(), n,
                frame0Index.data(), frame1Index.data(), descriptors0, n0, descriptors1, n1, thirdFrame.KeyPoints->data(),
                thirdFrame.Descriptors, n2, cameraIndex, ba ? ba->Outlier.data() : nullptr,
                ba ? ba->Position.data() : nullptr, ba ? ba->Rotation.data() : nullptr, ba ? ba->MeanSquareError : 0.f,
                &m_third, f.KeyPointOf.data(), f.Verdicts.data(), f.Distances.data(), f.Projections.data(),
                f.Unassociated.data(), f.Observations.data(), f.ObservationPoints.data(), f.ObservationCameras.data(),
                f.ObservationInformation.data(), nullptr, nullptr, nullptr));
        else
            check(mage_mono_init_third_frame(
                &m_settings, thirdFrame.Intrinsics.data(), positions.data(), rotations.data(), points.data(), n,
                frame0Index.data(), frame1Index.data(), descriptors0, n0, descriptors1, n1, thirdFrame.KeyPoints->data(),
                thirdFrame.Descriptors, n2, cameraIndex, &m_third, f.KeyPointOf.data(), f.Verdicts.data(),
                f.Distances.data(), f.Projections.data(), f.Unassociated.data(), f.Observations.data(),
                f.ObservationPoints.data(), f.ObservationCameras.data(), f.ObservationInformation.data(),
                f.Outliers.data(), m_device));
        if (m_third.status & MAGE_M3_STATUS_OVER_LIMIT)
            throw Error(MAGE_EUNSUPPORTED, "more than 4096 map points or third-frame keypoints");
        if (m_third.status & MAGE_M3_STATUS_BAD_INDEX) throw std::out_of_range("a map point names no keypoint");
        if (m_third.verdict != MAGE_M3_OK) return std::nullopt;
        const bool finished = m_device >= 0 || ba;
        const size_t na = finished ? m_third.n_associated : 0;
        std::copy(m_third.pos3, m_third.pos3 + 3, f.Position.begin());
        std::copy(m_third.r9, m_third.r9 + 9, f.Rotation.begin());
        std::copy(m_third.opt_pos3, m_third.opt_pos3 + 3, f.OptimizedPosition.begin());
        std::copy(m_third.opt_r9, m_third.opt_r9 + 9, f.OptimizedRotation.begin());
        f.Observations.resize(2 * na);
        f.ObservationPoints.resize(na);
        f.ObservationCameras.resize(na);
        f.ObservationInformation.resize(na);
        f.Outliers.resize(m_device >= 0 ? m_third.n_matched : 0);
        return f;
    }

    const mage_mono_init_result& LastResult() const { return m_last; }
    const std::vector<DMatch>& LastMatches() const { return m_matches; }
    const mage_mono_init_third_result& LastThirdResult() const { return m_third; }

private:
    mage_mono_init_settings m_settings;
    int m_device;
    mage_mono_init_result m_last{};
    mage_mono_init_third_result m_third{};
    std::vector<DMatch> m_matches;
};

// RelocalizationSettings (MageSettings.h:236-250) with its OrbMatcherSettings bag.
struct RelocalizationSettings {
    unsigned MinBruteForceCorrespondences{20}, MinRadiusMatchCorrespondences{15}, MinMapPoints{10};
    float RansacInliersPctRequired{0.4f}, BundleAdjustInliersPctRequired{0.4f}, RansacConfidence{0.6f};
    unsigned RoundRobinIterations{5}, RansacIterations{2}, BundleAdjustIterations{10};
    float SearchRadius{20.0f}, MaxBundleAdjustReprojectionError{8.0f}, MaxBundlePnPReprojectionError{8.0f};
    struct {
        int MaxHammingDistance{30}, MinHammingDifference{1};
    } OrbMatcherSettings;

    mage_reloc_settings ToC() const
    {
        mage_reloc_settings s{};
        s.struct_size = (uint32_t)sizeof(s);
        s.min_brute_force_correspondences = MinBruteForceCorrespondences;
        s.min_radius_match_correspondences = MinRadiusMatchCorrespondences;
        s.min_map_points = MinMapPoints;
        s.ransac_inliers_pct_required = RansacInliersPctRequired;
        s.bundle_adjust_inliers_pct_required = BundleAdjustInliersPctRequired;
        s.ransac_confidence = RansacConfidence;
        s.round_robin_iterations = RoundRobinIterations;
        s.ransac_iterations = RansacIterations;
        s.bundle_adjust_iterations = BundleAdjustIterations;
        s.search_radius = SearchRadius;
        s.max_bundle_adjust_reprojection_error = MaxBundleAdjustReprojectionError;
        s.max_bundle_pnp_reprojection_error = MaxBundlePnPReprojectionError;
        s.max_hamming_distance = OrbMatcherSettings.MaxHammingDistance;
        s.min_hamming_difference = OrbMatcherSettings.MinHammingDifference;
        return s;
    }
};

// A pose as the bundle adjustment takes it: view-space t and column-major R.
struct ViewPose {
    std::array<float, 3> Position{0.f, 0.f, 0.f};
    std::array<float, 9> Rotation{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
};

// The relocalisation of PoseEstimator (Tracking/PoseEstimator.h): PNPRansac over mage_reloc_pnp and
// TryEstimatePoseFromCandidates over mage_reloc_guided.
class PoseEstimator {
public:
    // device < 0 runs the CPU backend.
    explicit PoseEstimator(const RelocalizationSettings& settings, int device = 0)
        : m_settings(settings.ToC()), m_device(device)
    {
    }

    // PNPRansac (PoseEstimator.cpp:610-638) with the reference's arguments: calibration {cx, cy, fx,
    // fy} (undistorted), points3d[i] seen at points2d[i].  useExtrinsicGuess is accepted and ignored,
    // as OpenCV's RANSAC kernel ignores it.  false where the reference returns false (fewer than
    // five points, or no hypothesis with five inliers); else `pose` is the winning hypothesis and
    // `inliers` its inliers in point order WITHOUT those behind the camera — the caller's next step
    // (RemoveMapPointsThatAreBehind, :338) folded in; LastResult().n_inliers counts them all.
    // Throws Error (MAGE_EUNSUPPORTED) for more than 4096 points.
    bool PNPRansac(const std::array<float, 4>& calibration, const std::vector<std::array<float, 3>>& points3d,
                   const std::vector<std::array<float, 2>>& points2d, bool useExtrinsicGuess, float maxReprojectionError,
                   float ransacConfidence, unsigned numIterations, ViewPose& pose, std::vector<int>& inliers)
    {
        (void)useExtrinsicGuess;
        if (points3d.size() != points2d.size()) throw std::invalid_argument("one 2D point per 3D point");
        const uint32_t n = (uint32_t)points3d.size();
        mage_reloc_settings s = m_settings;
        s.min_brute_force_correspondences = 0;  // the gates around PNPRansac are the caller's
        s.ransac_inliers_pct_required = 0.f;
        s.max_bundle_pnp_reprojection_error = maxReprojectionError;
        s.ransac_confidence = ransacConfidence;
        s.ransac_iterations = numIterations;
        std::vector<float> map(4 * (size_t)n);
        std::vector<KeyPoint> kp(n);
        std::vector<DMatch> mm(n);
        for (uint32_t i = 0; i < n; i++) {
            std::copy(points3d[i].begin(), points3d[i].end(), &map[4 * (size_t)i]);
            map[4 * (size_t)i + 3] = 1.f;
            kp[i] = KeyPoint{};
            kp[i].x = points2d[i][0];
            kp[i].y = points2d[i][1];
            mm[i] = DMatch{};
            mm[i].query_idx = mm[i].train_idx = (int32_t)i;
        }
        const uint32_t cap = std::max<uint32_t>(n, 1);
        std::vector<uint32_t> idx(cap);
        std::vector<float> p3(3 * (size_t)cap), uv(2 * (size_t)cap), info(cap);
        m_last = mage_reloc_pnp_result{};
        if (m_device < 0)
            check(mage_reloc_pnp_host(&s, calibration.data(), map.data(), n, kp.data(), n, mm.data(), n, &m_last, idx.data(),
                                      cap, p3.data(), uv.data(), info.data(), nullptr));
        else
            check(mage_reloc_pnp(&s, calibration.data(), map.data(), n, kp.data(), n, mm.data(), n, &m_last, idx.data(),
                                 cap, p3.data(), uv.data(), info.data(), nullptr, m_device));
        if (m_last.status & MAGE_RP_STATUS_OVER_LIMIT) throw Error(MAGE_EUNSUPPORTED, "more than 4096 points");
        inliers.clear();
        if (m_last.verdict != MAGE_RP_OK) return false;
        std::copy(m_last.pos3, m_last.pos3 + 3, pose.Position.begin());
        std::copy(m_last.r9, m_last.r9 + 9, pose.Rotation.begin());
        inliers.assign(idx.begin(), idx.begin() + m_last.n_kept);
        return true;
    }

    const mage_reloc_pnp_result& LastResult() const { return m_last; }

    // A candidate keyframe as TryEstimatePoseFromCandidates reads it: per keypoint its map point
    // {x, y, z, information} (information <= 0: not associated), the keypoints and descriptors;
    // Order empty, or the associated keypoints in IterateAssociations' order; Intrinsics {cx, cy, fx,
    // fy} of the candidate for the bundle adjustments, all zero = the frame's.
    struct Candidate {
        std::vector<std::array<float, 4>> MapPoints;
        std::vector<KeyPoint> KeyPoints;
        std::vector<Descriptor> Descriptors;
        std::vector<int32_t> Order;
        std::array<float, 4> Intrinsics{0.f, 0.f, 0.f, 0.f};
    };
    // keyframe->AddAssociation(mapPoint, index) (:429-430): the candidate's keypoint whose map point
    // it is, and the frame's keypoint.
    struct Association {
        int32_t CandidateKeypoint, FrameKeypoint;
    };

    // TryEstimatePoseFromCandidates (PoseEstimator.cpp:219-437) behind IndexedMatch, whose matches
    // per candidate are given (queryIdx into the candidate, trainIdx into the frame): PNPRansac, the
    // first BundleAdjustPose, the guided search, the second BundleAdjustPose and the gates, for
    // every candidate on the GPU in one call.  Returns indexOfSuccess, the lowest candidate whose
    // pass succeeds (what the reference's round-robin returns, every round repeating the same
    // RANSAC), or -1; on success `pose` is the frame's pose and `associations` what it adds.
    // poseMaxHammingDist / poseMinHammingDifference are PoseEstimationSettings.OrbMatcherSettings.
    // Throws Error (MAGE_EUNSUPPORTED) on the CPU backend: the library has no host pose bundle
    // adjustment (mage_reloc_guided_host takes its outcome as an input).
    int TryEstimatePoseFromCandidates(const std::array<float, 4>& calibration, const std::vector<Candidate>& candidates,
                                      const std::vector<std::vector<DMatch>>& matches,
                                      const std::vector<KeyPoint>& keypoints, const std::vector<Descriptor>& descriptors,
                                      ViewPose& pose, std::vector<Association>& associations, int poseMaxHammingDist = 30,
                                      int poseMinHammingDifference = 1)
    {
        if (m_device < 0) throw Error(MAGE_EUNSUPPORTED, "TryEstimatePoseFromCandidates needs a GPU device");
        if (matches.size() != candidates.size()) throw std::invalid_argument("one match list per candidate");
        if (descriptors.size() != keypoints.size()) throw std::invalid_argument("one descriptor per keypoint");
        const uint32_t P = (uint32_t)candidates.size();
        associations.clear();
        m_guided.clear();
        m_frame = mage_reloc_frame_result{};
        m_frame.index = -1;
        if (P == 0) return -1;
        size_t pitch = 1, mcap = 1;
        bool ordered = false;
        for (uint32_t c = 0; c < P; c++) {
            const Candidate& k = candidates[c];
            if (k.KeyPoints.size() != k.MapPoints.size() || k.Descriptors.size() != k.MapPoints.size())
                throw std::invalid_argument("one map point slot and one descriptor per candidate keypoint");
            pitch = std::max({pitch, k.MapPoints.size(), k.Order.size()});
            mcap = std::max(mcap, matches[c].size());
            ordered = ordered || !k.Order.empty();
        }
        std::vector<float> map(4 * pitch * P, 0.f), bai(4 * (size_t)P);
        std::vector<KeyPoint> kfkp(pitch * P, KeyPoint{});
        std::vector<uint8_t> kfd(32 * pitch * P, 0);
        std::vector<int32_t> order(pitch * P, 0);
        std::vector<uint32_t> nkf(P), nord(P), nm(P);
        std::vector<DMatch> mm(mcap * P, DMatch{});
        for (uint32_t c = 0; c < P; c++) {
            const Candidate& k = candidates[c];
            const size_t n = k.MapPoints.size();
            nkf[c] = (uint32_t)n;
            for (size_t i = 0; i < n; i++) {
                std::copy(k.MapPoints[i].begin(), k.MapPoints[i].end(), &map[4 * (pitch * c + i)]);
                std::copy(k.Descriptors[i].begin(), k.Descriptors[i].end(), &kfd[32 * (pitch * c + i)]);
            }
            std::copy(k.KeyPoints.begin(), k.KeyPoints.end(), kfkp.begin() + pitch * c);
            // one order list needs them all: the default order is ascending keypoint index
            uint32_t no = 0;
            if (!k.Order.empty())
                for (int32_t v : k.Order) order[pitch * c + no++] = v;
            else
                for (size_t i = 0; i < n; i++)
                    if (k.MapPoints[i][3] > 0.f) order[pitch * c + no++] = (int32_t)i;
            nord[c] = no;
            const bool own = k.Intrinsics[2] != 0.f || k.Intrinsics[3] != 0.f;
            std::copy(own ? k.Intrinsics.begin() : calibration.begin(), own ? k.Intrinsics.end() : calibration.end(),
                      &bai[4 * (size_t)c]);
            nm[c] = (uint32_t)matches[c].size();
            std::copy(matches[c].begin(), matches[c].end(), mm.begin() + mcap * c);
        }
        const uint32_t cap = (uint32_t)pitch;
        m_guided.assign(P, mage_reloc_guided_result{});
        m_pnp.assign(P, mage_reloc_pnp_result{});
        std::vector<int32_t> assoc(2 * (size_t)cap * P);
        check(mage_reloc_guided(&m_settings, poseMaxHammingDist, poseMinHammingDifference, P, calibration.data(), bai.data(),
                                map.data(), kfkp.data(), kfd.data(), (uint32_t)pitch, nkf.data(),
                                ordered ? order.data() : nullptr, ordered ? nord.data() : nullptr,
                                keypoints.empty() ? nullptr : keypoints.data(),
                                descriptors.empty() ? nullptr : descriptors.front().data(), (uint32_t)keypoints.size(),
                                mm.data(), (uint32_t)mcap, nm.data(), cap, m_guided.data(), m_pnp.data(), &m_frame,
                                assoc.data(), m_device));
        if (m_frame.index < 0) return -1;
        std::copy(m_frame.pos3, m_frame.pos3 + 3, pose.Position.begin());
        std::copy(m_frame.r9, m_frame.r9 + 9, pose.Rotation.begin());
        const int32_t* a = &assoc[2 * (size_t)cap * (size_t)m_frame.index];
        for (uint32_t i = 0; i < m_frame.n_assoc; i++) associations.push_back(Association{a[2 * i], a[2 * i + 1]});
        return m_frame.index;
    }

    // The same from the vocabulary tree: IndexedMatch of every candidate's associated keypoints
    // against the frame with the relocaliser's OrbMatcherSettings (:279-289), then the call above.
    int TryEstimatePoseFromCandidates(const OnlineBowTree& bagOfWords, const std::array<float, 4>& calibration,
                                      const std::vector<Candidate>& candidates, const std::vector<KeyPoint>& keypoints,
                                      const std::vector<Descriptor>& descriptors, ViewPose& pose,
                                      std::vector<Association>& associations, int poseMaxHammingDist = 30,
                                      int poseMinHammingDifference = 1)
    {
        std::vector<std::vector<DMatch>> matches(candidates.size());
        for (size_t c = 0; c < candidates.size(); c++) {
            const Candidate& k = candidates[c];
            if (k.Descriptors.empty() || descriptors.empty() || k.Descriptors.size() > 4096 || descriptors.size() > 4096)
                continue;  // no match; a side over the limit is reported by the stage
            std::vector<bool> mask(k.MapPoints.size());
            for (size_t i = 0; i < mask.size(); i++) mask[i] = k.MapPoints[i][3] > 0.f;
            IndexedMatch(bagOfWords, k.Descriptors, descriptors, mask, std::vector<bool>(), m_settings.max_hamming_distance,
                         m_settings.min_hamming_difference, matches[c]);
        }
        return TryEstimatePoseFromCandidates(calibration, candidates, matches, keypoints, descriptors, pose, associations,
                                             poseMaxHammingDist, poseMinHammingDifference);
    }

    // Per candidate of the last call: the guided half's record and the PnP stage's.
    const std::vector<mage_reloc_guided_result>& LastCandidates() const { return m_guided; }
    const std::vector<mage_reloc_pnp_result>& LastCandidatesPnP() const { return m_pnp; }
    const mage_reloc_frame_result& LastFrame() const { return m_frame; }

private:
    mage_reloc_settings m_settings;
    int m_device;
    mage_reloc_pnp_result m_last{};
    std::vector<mage_reloc_guided_result> m_guided;
    std::vector<mage_reloc_pnp_result> m_pnp;
    mage_reloc_frame_result m_frame{};
};

struct BundlerParameters {
    bool ArePointsFixed{false};
};

// BundlerLib (Dependencies/BundlerLib/Include/BundlerLib.h:20-66).  The Set* calls buffer on
// the host; the problem is uploaded at the first StepBundleAdjustment.
class BundlerLib {
public:
    explicit BundlerLib(const BundlerParameters& params, int device = 0) : m_params(params)
    {
        check(mage_ba_create(params.ArePointsFixed ? 1 : 0, device, &m_handle));
    }
    ~BundlerLib() { mage_ba_destroy(m_handle); }
    BundlerLib(const BundlerLib&) = delete;
    BundlerLib& operator=(const BundlerLib&) = delete;

    void AllocateCameras(size_t count)
    {
        m_pos.assign(3 * count, 0.f);
        m_rot.assign(9 * count, 0.f);
        m_intr.assign(4 * count, 0.f);
        m_fixed.assign(count, 0);
        m_dirty = true;
    }
    // position: view-space t (3); orientation: Eigen::Map<const Matrix3f> data (column-major 9);
    // intrinsics: {cx, cy, fx, fy}
    void SetCameraPose(size_t idx, const float* position, const float* orientationColMajor, const float* intrinsics,
                       bool isFixed)
    {
        std::copy(position, position + 3, &m_pos[3 * idx]);
        std::copy(orientationColMajor, orientationColMajor + 9, &m_rot[9 * idx]);
        std::copy(intrinsics, intrinsics + 4, &m_intr[4 * idx]);
        m_fixed[idx] = isFixed ? 1 : 0;
        m_dirty = true;
    }
    void FixCameraPose(size_t idx, bool value)
    {
        m_fixed[idx] = value ? 1 : 0;
        if (!m_dirty) check(mage_ba_fix_camera(m_handle, (uint32_t)idx, value ? 1 : 0));
    }
    void AllocateMapPoints(size_t count)
    {
        m_points.assign(3 * count, 0.f);
        m_dirty = true;
    }
    void SetMapPoint(size_t idx, const float* point)
    {
        std::copy(point, point + 3, &m_points[3 * idx]);
        m_dirty = true;
    }
    void AllocateObservations(size_t count)
    {
        m_uv.assign(2 * count, 0.f);
        m_cam.assign(count, 0);
        m_pt.assign(count, 0);
        m_info.assign(count, 0.f);
        m_dirty = true;
    }
    void SetObservation(size_t idx, const float* position, size_t cameraIndex, size_t mapPointIndex,
                        float informationMatrixScalar)
    {
        m_uv[2 * idx] = position[0];
        m_uv[2 * idx + 1] = position[1];
        m_cam[idx] = (uint32_t)cameraIndex;
        m_pt[idx] = (uint32_t)mapPointIndex;
        m_info[idx] = informationMatrixScalar;
        m_dirty = true;
    }
    // Tether constraints (BundlerLib.cpp:229-257, 311-350); quaternions are (x, y, z, w).
    void AllocateFixedDistanceConstraints(size_t count) { m_teth[MAGE_TETHER_DISTANCE].resize(count); m_dirty = true; }
    void SetFixedDistanceConstraint(size_t idx, size_t cameraIndex1, size_t cameraIndex2, float distance = 1.0f,
                                    float weight = 1.0f)
    {
        m_teth[MAGE_TETHER_DISTANCE][idx] = {(uint32_t)cameraIndex1, (uint32_t)cameraIndex2, weight, {distance}};
        m_dirty = true;
    }
    void AllocateRelativeRotationConstraints(size_t count) { m_teth[MAGE_TETHER_ROTATION].resize(count); m_dirty = true; }
    void SetRelativeRotationConstraint(size_t idx, size_t cameraIndex1, size_t cameraIndex2, const float* deltaRotationXYZW,
                                       float weight = 1.0f)
    {
        Tether t{(uint32_t)cameraIndex1, (uint32_t)cameraIndex2, weight, {}};
        std::copy(deltaRotationXYZW, deltaRotationXYZW + 4, t.params);
        m_teth[MAGE_TETHER_ROTATION][idx] = t;
        m_dirty = true;
    }
    void AllocateRelativeTransformConstraints(size_t count) { m_teth[MAGE_TETHER_TRANSFORM].resize(count); m_dirty = true; }
    void SetRelativeTransformConstraint(size_t idx, size_t cameraIndex1, size_t cameraIndex2, const float* deltaPosition,
                                        const float* deltaRotationXYZW, float weight)
    {
        Tether t{(uint32_t)cameraIndex1, (uint32_t)cameraIndex2, weight, {}};
        std::copy(deltaPosition, deltaPosition + 3, t.params);
        std::copy(deltaRotationXYZW, deltaRotationXYZW + 4, t.params + 3);
        m_teth[MAGE_TETHER_TRANSFORM][idx] = t;
        m_dirty = true;
    }
    void SetCurrentLambda(float userLambda) { check(mage_ba_set_lambda(m_handle, userLambda)); }
    float GetCurrentLambda() const
    {
        float l = 0;
        check(mage_ba_get_lambda(m_handle, &l));
        return l;
    }
    // Runs one LM iteration per Huber width; returns the mean squared error of the kept edges
    // and appends the outlier observation indices.
    float StepBundleAdjustment(const std::vector<float>& huberWidthPerIteration, float maxErrorSquare,
                               std::vector<unsigned>& outliers)
    {
        upload();
        std::vector<uint32_t> out(std::max<size_t>(m_cam.size(), 1));
        uint32_t n = 0;
        float ms = 0;
        check(mage_ba_step(m_handle, huberWidthPerIteration.data(), (uint32_t)huberWidthPerIteration.size(),
                           maxErrorSquare, out.data(), (uint32_t)out.size(), &n, &ms));
        outliers.insert(outliers.end(), out.begin(), out.begin() + n);
        return ms;
    }
    void GetPose(size_t idx, float* position, float* orientationColMajor) const
    {
        std::vector<float> pos(m_pos.size()), rot(m_rot.size());
        check(mage_ba_get_poses(m_handle, pos.data(), rot.data()));
        std::copy(&pos[3 * idx], &pos[3 * idx] + 3, position);
        std::copy(&rot[9 * idx], &rot[9 * idx] + 9, orientationColMajor);
    }
    void GetPoint(size_t idx, float* position) const
    {
        std::vector<float> xyz(m_points.size());
        check(mage_ba_get_points(m_handle, xyz.data()));
        std::copy(&xyz[3 * idx], &xyz[3 * idx] + 3, position);
    }

private:
    void upload()
    {
        if (!m_dirty) return;
        check(mage_ba_set_cameras(m_handle, (uint32_t)m_fixed.size(), m_pos.data(), m_rot.data(), m_intr.data(),
                                  m_fixed.data()));
        check(mage_ba_set_points(m_handle, (uint32_t)(m_points.size() / 3), m_points.data()));
        check(mage_ba_set_observations(m_handle, (uint32_t)m_cam.size(), m_uv.data(), m_cam.data(), m_pt.data(),
                                       m_info.data()));
        static const int stride[3] = {1, 4, 7};
        for (uint32_t kind = 0; kind < 3; kind++) {
            const auto& v = m_teth[kind];
            std::vector<uint32_t> c1(v.size()), c2(v.size());
            std::vector<float> params(v.size() * stride[kind]), weight(v.size());
            for (size_t i = 0; i < v.size(); i++) {
                c1[i] = v[i].cam1;
                c2[i] = v[i].cam2;
                weight[i] = v[i].weight;
                std::copy(v[i].params, v[i].params + stride[kind], &params[i * stride[kind]]);
            }
            check(mage_ba_set_tethers(m_handle, kind, (uint32_t)v.size(), c1.data(), c2.data(), params.data(),
                                      weight.data()));
        }
        m_dirty = false;
    }

    struct Tether {
        uint32_t cam1, cam2;
        float weight;
        float params[7];
    };
    std::vector<Tether> m_teth[3];

    BundlerParameters m_params;
    mage_ba* m_handle = nullptr;
    bool m_dirty = true;
    std::vector<float> m_pos, m_rot, m_intr, m_points, m_uv, m_info;
    std::vector<uint8_t> m_fixed;
    std::vector<uint32_t> m_cam, m_pt;
};

// BoundingDepthSettings (MageSettings.h:216-223).
struct BoundingDepthSettings {
    float RegionOfInterestMinX{0.1f}, RegionOfInterestMinY{0.1f}, RegionOfInterestMaxX{0.9f}, RegionOfInterestMaxY{0.9f};
    float NearDepthSoftness{0.f}, FarDepthSoftness{0.f};

    mage_bounding_depth_settings ToC() const
    {
        mage_bounding_depth_settings s{};
        s.struct_size = (uint32_t)sizeof(s);
        s.region_of_interest_min_x = RegionOfInterestMinX;
        s.region_of_interest_min_y = RegionOfInterestMinY;
        s.region_of_interest_max_x = RegionOfInterestMaxX;
        s.region_of_interest_max_y = RegionOfInterestMaxY;
        s.near_depth_softness = NearDepthSoftness;
        s.far_depth_softness = FarDepthSoftness;
        return s;
    }
};

using ProjectedPoint = mage_projected_point;  // Data/Data.h:112-124

// InternalDepth (Data/Data.h): the two plane depths and the sparse depth map it owns.
struct InternalDepth {
    static constexpr float INVALID_DEPTH = MAGE_INVALID_DEPTH;
    float NearPlaneDepth{INVALID_DEPTH}, FarPlaneDepth{INVALID_DEPTH};
    std::vector<ProjectedPoint> SparseDepth;
    mage_depth_result Result{};  // the counts and the status bits
};

// CalculateBoundingPlaneDepthsForKeyframe (Tracking/BoundingPlaneDepths.cpp:16-87).  The keyframe is
// given as what the routine reads of it: the view matrix in the bundler form, the undistorted
// calibration {cx, cy, fx, fy}, the image size, the keypoints, and per associated map point its
// position with the id's bits {x, y, z, id} and the index of its keypoint (GetAssociatedKeyPoint).
// device < 0 runs the CPU backend.  Throws Error (MAGE_EUNSUPPORTED) for more than
// MAGE_BD_MAX_POINTS map points and std::out_of_range for a keypoint index outside the keypoints.
inline InternalDepth CalculateBoundingPlaneDepthsForKeyframe(const ViewPose& pose, const std::array<float, 4>& calibration,
                                                             uint32_t width, uint32_t height,
                                                             const std::vector<KeyPoint>& keypoints,
                                                             const std::vector<std::array<float, 4>>& mapPoints,
                                                             const std::vector<int32_t>& associatedKeypoints,
                                                             const BoundingDepthSettings& settings, int device = 0)
{
    if (mapPoints.size() != associatedKeypoints.size()) throw std::invalid_argument("one keypoint index per map point");
    const mage_bounding_depth_settings s = settings.ToC();
    const uint32_t n = (uint32_t)mapPoints.size();
    InternalDepth d;
    d.SparseDepth.resize(n);
    const float* map = n ? mapPoints[0].data() : nullptr;
    if (device < 0)
        check(mage_bounding_plane_depths_host(&s, pose.Position.data(), pose.Rotation.data(), calibration.data(), width,
                                              height, keypoints.data(), (uint32_t)keypoints.size(), map,
                                              associatedKeypoints.data(), n, n, &d.Result, d.SparseDepth.data()));
    else
        check(mage_bounding_plane_depths(&s, pose.Position.data(), pose.Rotation.data(), calibration.data(), width, height,
                                         keypoints.data(), (uint32_t)keypoints.size(), map, associatedKeypoints.data(), n,
                                         n, &d.Result, d.SparseDepth.data(), device));
    if (d.Result.status & MAGE_BD_STATUS_OVER_LIMIT) throw Error(MAGE_EUNSUPPORTED, "more than 8192 map points in a frame");
    if (d.Result.status & MAGE_BD_STATUS_BAD_INDEX) throw std::out_of_range("a map point names no keypoint");
    d.NearPlaneDepth = d.Result.near_plane;
    d.FarPlaneDepth = d.Result.far_plane;
    return d;
}

// VolumeOfInterestSettings (MageSettings.h:290-307).
struct VolumeOfInterestSettings {
    float Threshold{0.5f};
    int Iterations{3}, VoxelCountFloor{16000};
    float AwayProminence{1.2f}, TowardProminence{0.1f}, SideProminence{1.f};
    float KernelAngleXRads{1.04719755f}, KernelAngleYRads{0.69813170f};  // deg2rad(60), deg2rad(40)
    float KernelPitchRads{0.f}, KernelRollRads{0.f}, KernelYawRads{0.08726646f};  // deg2rad(5)
    float KernelDepthModifier{1.f};

    mage_voi_settings ToC() const
    {
        mage_voi_settings s{};
        s.struct_size = (uint32_t)sizeof(s);
        s.threshold = Threshold;
        s.iterations = Iterations;
        s.voxel_count_floor = VoxelCountFloor;
        s.away_prominence = AwayProminence;
        s.toward_prominence = TowardProminence;
        s.side_prominence = SideProminence;
        s.kernel_angle_x_rads = KernelAngleXRads;
        s.kernel_angle_y_rads = KernelAngleYRads;
        s.kernel_pitch_rads = KernelPitchRads;
        s.kernel_roll_rads = KernelRollRads;
        s.kernel_yaw_rads = KernelYawRads;
        s.kernel_depth_modifier = KernelDepthModifier;
        return s;
    }
};

// AxisAlignedVolume (Data/Data.h).
struct AxisAlignedVolume {
    std::array<float, 3> Min{}, Max{};
};

// What VOIKeyframe's constructor reads (VolumeOfInterest.cpp:45-61): the world-from-camera matrix
// (3 x 4, row-major: ToPose(WorldPosition)'s inverse view matrix) and the frame's plane depths.
struct VOIKeyframe {
    std::array<float, 12> WorldFromCamera;
    float NearDepth, FarDepth;
};

// CalculateVolumeOfInterest (VolumeOfInterest.cpp:88-259): false without keyframes (`voi` untouched),
// true otherwise, as the reference returns; `result`, when given, receives the status
// (MAGE_VOI_DEGENERATE / MAGE_VOI_EMPTY: `voi` holds what the last level that passed left) and
// `trace` the per-level records.  device < 0 runs the CPU backend.
inline bool CalculateVolumeOfInterest(const std::vector<VOIKeyframe>& keyframes, const VolumeOfInterestSettings& voiSettings,
                                      AxisAlignedVolume& voi, mage_voi_result* result = nullptr,
                                      std::vector<mage_voi_level>* trace = nullptr, int device = 0)
{
    const mage_voi_settings s = voiSettings.ToC();
    const uint32_t n = (uint32_t)keyframes.size();
    std::vector<float> m(12 * (size_t)n), nf(2 * (size_t)n);
    for (uint32_t k = 0; k < n; k++) {
        std::copy(keyframes[k].WorldFromCamera.begin(), keyframes[k].WorldFromCamera.end(), &m[12 * (size_t)k]);
        nf[2 * (size_t)k] = keyframes[k].NearDepth;
        nf[2 * (size_t)k + 1] = keyframes[k].FarDepth;
    }
    mage_voi_result r{};
    std::vector<mage_voi_level> levels((size_t)std::max(voiSettings.Iterations, 0));
    if (device < 0)
        check(mage_volume_of_interest_host(&s, m.data(), nf.data(), nullptr, 0, nullptr, n, &r, levels.data()));
    else
        check(mage_volume_of_interest(&s, m.data(), nf.data(), nullptr, 0, nullptr, n, &r, levels.data(), device));
    if (result) *result = r;
    if (r.status == MAGE_VOI_NO_KEYFRAMES) return false;
    if (trace) *trace = levels;
    std::copy(r.min, r.min + 3, voi.Min.begin());
    std::copy(r.max, r.max + 3, voi.Max.begin());
    return true;
}

}  // namespace hot
}  // namespace mage
