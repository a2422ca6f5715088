// rolo_nodes_hip.hpp — header-only C++ host mirrors of the three front-end node cores of sdwyc/ROLO over the C ABI
// of librolo_hip.so (include/rolo_hip.h). Class, method and member names follow the reference so that the node
// sources keep reading the way they do; everything ROS (subscribers, publishers, messages) stays in the node.
//
//   rolo::ImageProjection    projectPointCloud() + cloudExtraction()                 src/imageProjection.cpp:399-505
//   rolo::FeatureExtraction  calculateSmoothness() + markOccludedPoints() + extractFeatures()
//                                                                                     src/featureExtraction.cpp:87-266
//   rolo::LidarOdometry      odometryHandler() / cloudHandler()                       src/lidarOdometry.cpp:440-446, 503-570
//                            + the fused device-resident path frame() / submit() / collect() (rolo_odom_frame & co)
// and of the back end's mapping node:
//   rolo::MapOptimization    laserCloudInfoHandler()                                  src/backMapping.cpp:420-457 (rolo_mapper_scan)
//
// Data are plain arrays with the layout of rolo/CloudInfoStamp (msg/CloudInfoStamp.msg:1-28): int32 startRingIndex /
// endRingIndex / pointColInd, float32 pointRange, feature clouds as n x 4 floats (x, y, z, intensity).
// Error behaviour: the reference nodes log and drop the frame or shut down; these classes throw rolo::Error (a
// std::runtime_error carrying the ROLO_E* code) and leave the policy to the node.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "rolo_hip.h"

namespace rolo {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& where) : std::runtime_error(where + ": " + (rolo_last_error() ? rolo_last_error() : "")), code(c) {}
};
inline int check(int rc, const char* where) { if (rc < 0) throw Error(rc, where); return rc; }

// one registration context (one HIP stream) — RAII
class Context {
public:
  explicit Context(int device = 0) { check(rolo_ctx_create(device, &ctx_), "rolo_ctx_create"); }
  ~Context() { rolo_ctx_destroy(ctx_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  rolo_ctx* get() const { return ctx_; }
private:
  rolo_ctx* ctx_ = nullptr;
};

// config/params.yaml:20-36 under the names of include/rolo/utility.h (ParamLoader)
struct FrontParams : rolo_front_params {
  FrontParams() { rolo_front_default_params(this); }
  FrontParams(int N_SCAN, int Horizon_SCAN, int downsampleRate = 1, float lidarMinRange = 2.0f, float lidarMaxRange = 1000.0f,
              float edgeThreshold = 0.8f, float surfThreshold = 0.1f, float odometrySurfLeafSize = 0.4f) {
    n_scan = N_SCAN; horizon_scan = Horizon_SCAN; downsample_rate = downsampleRate; lidar_min_range = lidarMinRange;
    lidar_max_range = lidarMaxRange; edge_threshold = edgeThreshold; surf_threshold = surfThreshold; odometry_surf_leaf_size = odometrySurfLeafSize;
  }
};

// The per-frame arrays ImageProjection publishes in rolo/cloud_info
struct CloudInfo {
  std::vector<int32_t> startRingIndex, endRingIndex, pointColInd;
  std::vector<float> pointRange;
  std::vector<float> extractedCloud;  // cloud_projected: N x 4 (x, y, z, intensity = ring * z, imageProjection.cpp:410)
  int n_valid = 0;
};

class ImageProjection {
public:
  ImageProjection(Context& ctx, const FrontParams& p) : ctx_(ctx), p_(p) {}
  // deskewCloudInfo() + deskewPoint() (:266-396) for the next projectPointCloud: odomIncreRoll/Pitch/Yaw, scanPeriod,
  // odomTimeDiff and rel_time[i] = fabs(point.time) of raw point i (host array of n values)
  void setDeskew(const float odomIncreRPY[3], float scanPeriod, double odomTimeDiff, const float* rel_time, int n, bool deskewEnabled = true) {
    rolo_deskew d{deskewEnabled ? 1 : 0, {odomIncreRPY[0], odomIncreRPY[1], odomIncreRPY[2]}, scanPeriod, odomTimeDiff};
    check(rolo_front_set_deskew(ctx_.get(), &d, rel_time, n, 0), "rolo_front_set_deskew");
  }
  // projectPointCloud() + cloudExtraction(): `pts` = n records of `stride` floats (x, y, z first), `ring` the ring field
  const CloudInfo& projectPointCloud(const float* pts, int stride, const uint16_t* ring, int n) {
    const size_t npix = (size_t)p_.n_scan * p_.horizon_scan;
    info_.startRingIndex.assign(p_.n_scan, 0); info_.endRingIndex.assign(p_.n_scan, 0);
    info_.pointColInd.assign(npix, 0); info_.pointRange.assign(npix, 0.f); info_.extractedCloud.assign(npix * 4, 0.f);
    check(rolo_project_frame(ctx_.get(), &p_, pts, stride, ring, n, info_.extractedCloud.data(), info_.pointColInd.data(), info_.pointRange.data(),
                             info_.startRingIndex.data(), info_.endRingIndex.data(), nullptr, &info_.n_valid), "rolo_project_frame");
    info_.pointColInd.resize(info_.n_valid); info_.pointRange.resize(info_.n_valid); info_.extractedCloud.resize((size_t)info_.n_valid * 4);
    return info_;
  }
  const CloudInfo& cloudInfo() const { return info_; }
private:
  Context& ctx_;
  FrontParams p_;
  CloudInfo info_;
};

class FeatureExtraction {
public:
  FeatureExtraction(Context& ctx, const FrontParams& p) : ctx_(ctx), p_(p) {}
  // runs on the arrays the preceding ImageProjection::projectPointCloud left on the device (same Context)
  void extractFeatures(int n_valid) {
    cornerCloud.assign((size_t)(n_valid > 0 ? n_valid : 1) * 4, 0.f); surfaceCloud.assign((size_t)(n_valid > 0 ? n_valid : 1) * 4, 0.f);
    int nc = 0, ns = 0;
    check(rolo_extract_features(ctx_.get(), &p_, cornerCloud.data(), &nc, surfaceCloud.data(), &ns, nullptr, nullptr, nullptr), "rolo_extract_features");
    cornerCloud.resize((size_t)nc * 4); surfaceCloud.resize((size_t)ns * 4);
  }
  std::vector<float> cornerCloud, surfaceCloud;  // extracted_corner / extracted_surface: n x 4
private:
  Context& ctx_;
  FrontParams p_;
};

class LidarOdometry {
public:
  // status of a frame, as rolo_odom_cloud returns it
  enum Status { FirstFrame = 0, Gated = 1, Registered = 2 };

  explicit LidarOdometry(Context& ctx, float CT_lambda = 0.3f, double polar_theta = 0.175, double polar_phi = 0.175, double polar_r = 2.0) : ctx_(ctx) {
    rolo_params P; rolo_default_params(&P);
    P.voxel_type = ROLO_VOXEL_POLAR;  // rot_vgicp.setPolarResolution(0.175, 0.175, 2.0), lidarOdometry.cpp:462
    P.polar_resolution[0] = polar_theta; P.polar_resolution[1] = polar_phi; P.polar_resolution[2] = polar_r;
    check(rolo_set_params(ctx_.get(), &P), "rolo_set_params");
    check(rolo_odom_create(ctx_.get(), CT_lambda, &odom_), "rolo_odom_create");
  }
  ~LidarOdometry() { rolo_odom_destroy(odom_); }
  LidarOdometry(const LidarOdometry&) = delete;
  LidarOdometry& operator=(const LidarOdometry&) = delete;

  void odometryHandler(double stamp) { check(rolo_odom_backend_odometry(odom_, stamp), "rolo_odom_backend_odometry"); }  // :440-446
  // :503-570 between fromROSMsg and pubMessage; clouds n x 4 floats
  Status cloudHandler(double stamp, const std::vector<float>& cornerCloud, const std::vector<float>& surfaceCloud) {
    return (Status)check(rolo_odom_cloud(odom_, stamp, cornerCloud.data(), (int)(cornerCloud.size() / 4), surfaceCloud.data(), (int)(surfaceCloud.size() / 4),
                                         LaserOdomPose.data(), Rotation.data(), Translation.data()), "rolo_odom_cloud");
  }
  // the three node cores fused, device-resident (raw frame -> pose)
  Status frame(const FrontParams& p, double stamp, const float* pts, int stride, const uint16_t* ring, int n, bool on_device = false) {
    return (Status)check(rolo_odom_frame(odom_, &p, stamp, pts, stride, ring, n, on_device ? 1 : 0, LaserOdomPose.data(), Rotation.data(), Translation.data(),
                                         counts.data()), "rolo_odom_frame");
  }
  void submit(const FrontParams& p, double stamp, const float* pts, int stride, const uint16_t* ring, int n, bool on_device = false) {
    check(rolo_odom_submit(odom_, &p, stamp, pts, stride, ring, n, on_device ? 1 : 0), "rolo_odom_submit");
  }
  // submit() from the payload of the sensor_msgs/PointCloud2 itself (field offsets from msg.fields): no host-side extraction
  void submitMsg(const FrontParams& p, double stamp, const uint8_t* data, const rolo_cloud_layout& layout, int n_points, bool on_device = false) {
    check(rolo_odom_submit_msg(odom_, &p, stamp, data, &layout, n_points, on_device ? 1 : 0), "rolo_odom_submit_msg");
  }
  Status collect() { return (Status)check(rolo_odom_collect(odom_, LaserOdomPose.data(), Rotation.data(), Translation.data(), counts.data()), "rolo_odom_collect"); }
  // de-skew of the next submit() / frame() (see ImageProjection::setDeskew)
  void setDeskew(const float odomIncreRPY[3], float scanPeriod, double odomTimeDiff, const float* rel_time, int n, bool deskewEnabled = true) {
    rolo_deskew d{deskewEnabled ? 1 : 0, {odomIncreRPY[0], odomIncreRPY[1], odomIncreRPY[2]}, scanPeriod, odomTimeDiff};
    check(rolo_odom_set_deskew(odom_, &d, rel_time, n, 0), "rolo_odom_set_deskew");
  }
  // extracted_corner ++ extracted_surface of the last collected fused frame (n x 4 floats, corners first)
  void getFeatures(std::vector<float>& features, int& n_corner, int& n_surface) {
    check(rolo_odom_get_features(odom_, nullptr, 0, &n_corner, &n_surface), "rolo_odom_get_features");
    features.assign((size_t)(n_corner + n_surface > 0 ? n_corner + n_surface : 1) * 4, 0.f);
    check(rolo_odom_get_features(odom_, features.data(), n_corner + n_surface, &n_corner, &n_surface), "rolo_odom_get_features");
  }
  void setReuseCovariances(bool on) { check(rolo_odom_set_option(odom_, ROLO_ODOM_REUSE_COVARIANCES, on ? 1 : 0), "rolo_odom_set_option"); }

  std::array<float, 6> LaserOdomPose{};   // x, y, z, roll, pitch, yaw — what pubMessage publishes (:680-684)
  std::array<double, 9> Rotation{};       // frame-to-frame step, row-major
  std::array<double, 3> Translation{};
  std::array<int, 3> counts{};            // N, n_corner, n_surface of the last fused frame
private:
  Context& ctx_;
  rolo_odom* odom_ = nullptr;
};

// rolo/mapping* of include/rolo/utility.h:320-343 under their own names
struct MapperParams : rolo_mapper_params {
  MapperParams() { rolo_mapper_default_params(this); }
};

// mapOptimization (src/backMapping.cpp): laserCloudInfoHandler :420-457 as one call per CloudInfoStamp (rolo_mapper_scan). The key map, the scan-to-submap
// context and the pose graph belong to the object; keymap() / graph() lend them to the loop-closure, Scan Context, global-map and ground-prior calls between
// scans. The reference's mtx stays with the node: one thread at a time.
class MapOptimization {
public:
  explicit MapOptimization(int device = 0, const MapperParams& params = MapperParams()) { check(rolo_mapper_create(device, &params, &mapper_), "rolo_mapper_create"); }
  ~MapOptimization() { rolo_mapper_destroy(mapper_); }
  MapOptimization(const MapOptimization&) = delete;
  MapOptimization& operator=(const MapOptimization&) = delete;

  // :420-457 between fromROSMsg and the publishers. laserCloudCornerLast / laserCloudSurfLast (extracted_surface ++ extracted_normal, :430): n x 4 floats;
  // cloud_projected may be empty; initialGuess = initialGuessRoll / Pitch / Yaw / X / Y / Z when odomAvailable. Returns false when the interval gate held the scan
  bool laserCloudInfoHandler(double timeLaserInfoCur, const std::vector<float>& laserCloudCornerLast, const std::vector<float>& laserCloudSurfLast,
                             const std::vector<float>& cloud_projected = {}, const float* initialGuess = nullptr, bool odomAvailable = false) {
    check(rolo_mapper_scan(mapper_, timeLaserInfoCur, laserCloudCornerLast.data(), (int)(laserCloudCornerLast.size() / 4), laserCloudSurfLast.data(),
                           (int)(laserCloudSurfLast.size() / 4), cloud_projected.empty() ? nullptr : cloud_projected.data(), (int)(cloud_projected.size() / 4), 0,
                           initialGuess, odomAvailable ? 1 : 0, &result), "rolo_mapper_scan");
    if (!result.processed) return false;
    for (int k = 0; k < 6; k++) transformTobeMapped[k] = result.transformTobeMapped[k];
    isDegenerate = result.s2m.degenerate != 0;
    return true;
  }
  // the same on device clouds of the mapper's device whose writers the caller has waited for
  bool laserCloudInfoHandlerDevice(double timeLaserInfoCur, const float* d_corner, int n_corner, const float* d_surf, int n_surf, const float* d_raw, int n_raw,
                                   const float* initialGuess = nullptr, bool odomAvailable = false) {
    check(rolo_mapper_scan(mapper_, timeLaserInfoCur, d_corner, n_corner, d_surf, n_surf, d_raw, n_raw, 1, initialGuess, odomAvailable ? 1 : 0, &result), "rolo_mapper_scan");
    if (!result.processed) return false;
    for (int k = 0; k < 6; k++) transformTobeMapped[k] = result.transformTobeMapped[k];
    isDegenerate = result.s2m.degenerate != 0;
    return true;
  }
  // loopIndexQueue / loopPoseQueue / loopNoiseQueue .push_back (:2388-2392; cauchy_k > 0: the Robust noise of :2468-2470), priorIndexQueue &c (:2129-2133)
  void queueLoop(int indexFrom, int indexTo, const double poseBetween[16], const double variances[6], double cauchy_k = 0.0) {
    check(rolo_mapper_queue_loop(mapper_, indexFrom, indexTo, poseBetween, variances, cauchy_k), "rolo_mapper_queue_loop");
  }
  void queuePrior(int indexFrom, int indexTo, const double poseBetween[16], const double variances[6]) {
    check(rolo_mapper_queue_prior(mapper_, indexFrom, indexTo, poseBetween, variances), "rolo_mapper_queue_prior");
  }
  // cloudKeyPoses6D: n x 6 floats (roll, pitch, yaw, x, y, z) and the stamps
  int cloudKeyPoses6D(std::vector<float>& pose6, std::vector<double>& time) {
    const int n = check(rolo_mapper_get_keyposes(mapper_, nullptr, nullptr, 0), "rolo_mapper_get_keyposes");
    pose6.assign((size_t)(n > 0 ? n : 1) * 6, 0.f); time.assign((size_t)(n > 0 ? n : 1), 0.0);
    check(rolo_mapper_get_keyposes(mapper_, pose6.data(), time.data(), n), "rolo_mapper_get_keyposes");
    pose6.resize((size_t)n * 6); time.resize((size_t)n);
    return n;
  }
  // laserCloudCornerLastDS / laserCloudSurfLastDS of the last processed scan
  void lastScanDS(std::vector<float>& laserCloudCornerLastDS, std::vector<float>& laserCloudSurfLastDS) {
    int cnt[2] = {0, 0};
    check(rolo_mapper_get_scan(mapper_, nullptr, 0, nullptr, 0, cnt), "rolo_mapper_get_scan");
    laserCloudCornerLastDS.assign((size_t)(cnt[0] > 0 ? cnt[0] : 1) * 4, 0.f); laserCloudSurfLastDS.assign((size_t)(cnt[1] > 0 ? cnt[1] : 1) * 4, 0.f);
    check(rolo_mapper_get_scan(mapper_, laserCloudCornerLastDS.data(), cnt[0], laserCloudSurfLastDS.data(), cnt[1], nullptr), "rolo_mapper_get_scan");
    laserCloudCornerLastDS.resize((size_t)cnt[0] * 4); laserCloudSurfLastDS.resize((size_t)cnt[1] * 4);
  }
  // publishFrames :1405-1414 — what pubRecentKeyFrame gets
  void registeredKeyFrame(std::vector<float>& cloudOut) {
    int cnt[2] = {0, 0};
    check(rolo_mapper_get_scan(mapper_, nullptr, 0, nullptr, 0, cnt), "rolo_mapper_get_scan");
    cloudOut.assign((size_t)(cnt[0] + cnt[1] > 0 ? cnt[0] + cnt[1] : 1) * 4, 0.f);
    const int n = check(rolo_mapper_get_registered(mapper_, cloudOut.data(), cnt[0] + cnt[1]), "rolo_mapper_get_registered");
    cloudOut.resize((size_t)n * 4);
  }
  // :1416-1424 — what pubCloudRegisteredRaw gets; n_raw: the size of the cloud_projected handed to the last scan
  void registeredRaw(std::vector<float>& cloudOut, int n_raw) {
    cloudOut.assign((size_t)(n_raw > 0 ? n_raw : 1) * 4, 0.f);
    const int n = check(rolo_mapper_get_registered_raw(mapper_, cloudOut.data(), n_raw), "rolo_mapper_get_registered_raw");
    cloudOut.resize((size_t)n * 4);
  }
  rolo_keymap* keymap() const { return rolo_mapper_keymap(mapper_); }   // borrowed
  rolo_pgo* graph() const { return rolo_mapper_pgo(mapper_); }          // borrowed
  rolo_mapper* get() const { return mapper_; }

  std::array<float, 6> transformTobeMapped{};   // roll, pitch, yaw, x, y, z
  bool isDegenerate = false;
  rolo_mapper_result result{};                  // of the last laserCloudInfoHandler: incremental6, the stats, the key frame, the graph's optimise
private:
  rolo_mapper* mapper_ = nullptr;
};

}  // namespace rolo
