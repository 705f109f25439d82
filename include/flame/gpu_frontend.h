// include/flame/gpu_frontend.h -- the feature pipeline of flame::Flame::update() on the GPU: detection on a cell grid and
// epipolar inverse-depth tracking (libflame_hip.so, flame_hip_frontend_*; the algorithm: DESIGN.md "Feature front end").
//
//   flame::Flame sensor(width, height, K, Kinv, params);
//   flame::GpuFrontEnd features(width, height, K, params);
//   sensor.setFrontEnd(features.frontEnd());
//   sensor.update(time, img_id, pose, gray, is_poseframe);   // reference src/flame_offline_tum.cc:578-579
//
// frontEnd() binds `track`, `updatePoseFramePoses`, `prunePoseFrames` and `reportStats` (the tracking stat keys num_idepth_updates
// / num_fail_*) to this object (which must outlive the Flame it feeds); `triangulate` stays empty, so the library's GPU Delaunay triangulation runs.  `track` hands every emitted feature of the frame
// to Flame (whose variance gate selects the ones that enter the graph) and fails the frame when fewer than three are emitted.
// Poses are T_world_cam; they cross into the library as row-major [R|t] in double, made from the unit quaternion and the
// translation of SE3f (Sophus::SE3f when present, the fallback struct otherwise).  Nothing throws; a failure leaves its code
// in lastError() (and the frame fails, which Flame reports like any failed update).
#pragma once
#include <cmath>
#include <cstdint>
#include <functional>
#include <vector>

#include "../flame_hip.h"
#include "flame.h"
#include "params.h"
#include "types.h"

namespace flame {

class GpuFrontEnd {
 public:
  GpuFrontEnd(int width, int height, const Matrix3f& K, const Params& params = Params(), int max_features = 4096,
              int max_poseframes = 16)
      : width_(width), height_(height) {
    float Kr[9];
    toRowMajor(K, Kr);
    flame_hip_frontend_default_params(&fparams_);
    fparams_.detection_win_size = params.detection_win_size;
    fparams_.min_grad_mag = params.min_grad_mag;
    fparams_.win_size = params.zparams.win_size;
    fparams_.epipolar_line_var = params.zparams.epipolar_line_var;
    fparams_.max_dropouts = params.max_dropouts;
    last_error_ = flame_hip_frontend_create(&handle_, params.hip_device, width, height, Kr, max_features, max_poseframes);
    if (last_error_) handle_ = nullptr;
  }
  ~GpuFrontEnd() { flame_hip_frontend_destroy(handle_); }
  GpuFrontEnd(const GpuFrontEnd&) = delete;
  GpuFrontEnd& operator=(const GpuFrontEnd&) = delete;

  // the front end's own parameters (search clamp, prior of a new feature, match threshold): change before the first frame
  flame_hip_frontend_params& frontendParams() { return fparams_; }
  int lastError() const { return last_error_; }
  flame_hip_frontend* handle() const { return handle_; }

  FrontEnd frontEnd() {
    FrontEnd fe;
    fe.track = [this](const FrameInput& in, FeatureSet* out) { return track(in, out); };
    fe.updatePoseFramePoses = [this](const std::vector<uint32_t>& ids, const std::vector<SE3f>& poses) { updatePoseFramePoses(ids, poses); };
    fe.prunePoseFrames = [this](const std::vector<uint32_t>& ids) { prunePoseFrames(ids); };
    fe.reportStats = [this](utils::StatsTracker* stats) { reportStats(stats); };
    return fe;
  }

  bool track(const FrameInput& in, FeatureSet* out) {
    if (!handle_) return false;  // (lastError() still holds why the handle could not be made)
    if (!in.img || !out || in.img->rows != height_ || in.img->cols != width_) return fail(FLAME_HIP_ERR_ARG);
    double T[12];
    toRt(in.pose, T);
    const uint8_t* row0 = in.img->ptr<uint8_t>(0);
    const int32_t pitch = height_ > 1 ? static_cast<int32_t>(in.img->ptr<uint8_t>(1) - row0) : width_;
    int32_t n = 0;
    int rc = flame_hip_frontend_track(handle_, &fparams_, row0, pitch, in.img_id, T, in.is_poseframe ? 1 : 0, &n);
    if (rc) return fail(rc);
    static_assert(sizeof(Point2f) == 2 * sizeof(float), "boundary types are packed");
    out->vtx.resize(static_cast<size_t>(n));
    out->idepth_mu.resize(static_cast<size_t>(n));
    out->idepth_var.resize(static_cast<size_t>(n));
    out->prediction.clear();
    rc = flame_hip_frontend_features(handle_, n, n ? reinterpret_cast<float*>(out->vtx.data()) : nullptr, out->idepth_mu.data(),
                                     out->idepth_var.data(), nullptr, nullptr);
    if (rc) return fail(rc);
    last_error_ = 0;
    return n >= 3;
  }

  void updatePoseFramePoses(const std::vector<uint32_t>& ids, const std::vector<SE3f>& poses) {
    if (!handle_ || ids.size() != poses.size()) return;
    std::vector<double> T(12 * ids.size());
    for (size_t i = 0; i < ids.size(); ++i) toRt(poses[i], &T[12 * i]);
    last_error_ = flame_hip_frontend_set_poses(handle_, static_cast<int32_t>(ids.size()), ids.data(), T.data());
  }
  void prunePoseFrames(const std::vector<uint32_t>& keep_ids) {
    if (!handle_) return;
    last_error_ = flame_hip_frontend_prune(handle_, static_cast<int32_t>(keep_ids.size()), keep_ids.data());
  }

  // The tracking stats FlameStats carries (reference src/utils.cc:124-129), from the counts of the frame just tracked
  // (flame_hip_frontend_info): features whose idepth was updated, features that died of too many dropouts, ambiguous matches,
  // matches above the cost threshold.  `num_fail_max_var` is Flame's own (its variance gate); `num_fail_ref_patch_grad` has no
  // counterpart in this front end's statement (DESIGN.md 5.3 tests no reference-patch gradient) and stays unset.
  void reportStats(utils::StatsTracker* stats) const {
    if (!handle_ || !stats) return;
    static const char* const kKeys[4][2] = {{"num_idepth_updates", "ok"}, {"num_fail_max_dropouts", "died"},
                                            {"num_fail_ambiguous_match", "ambiguous"}, {"num_fail_max_cost", "bad_match"}};
    for (int k = 0; k < 4; ++k) {
      int64_t v = 0;
      if (flame_hip_frontend_info(handle_, kKeys[k][1], &v) == 0) stats->set(kKeys[k][0], static_cast<double>(v));
    }
  }

  // [R|t], row-major 3x4 in double (flame/types.h poseToRt, shared with Flame's prediction stage)
  static void toRt(const SE3f& pose, double T[12]) { poseToRt(pose, T); }

 private:
  bool fail(int code) {
    last_error_ = code;
    return false;
  }
  int width_, height_;
  flame_hip_frontend_params fparams_;
  flame_hip_frontend* handle_ = nullptr;
  int last_error_ = 0;
};

}  // namespace flame
