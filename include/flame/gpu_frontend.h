// include/flame/gpu_frontend.h -- the feature pipeline of flame::Flame::update() on the GPU: detection on a cell grid and
// epipolar inverse-depth tracking (libflame_hip.so, flame_hip_frontend_*; the algorithm: DESIGN.md "Feature front end").
//
//   flame::Flame sensor(width, height, K, Kinv, params);
//   flame::GpuFrontEnd features(width, height, K, params);
//   sensor.setFrontEnd(features.frontEnd());
//   sensor.update(time, img_id, pose, gray, is_poseframe);   // reference src/flame_offline_tum.cc:578-579
//
// frontEnd() binds `track`, `updatePoseFramePoses`, `prunePoseFrames`, `reportStats` (the tracking stat keys num_idepth_updates
// / num_fail_*) and `debugImage` (the Detections / Matches pictures behind Flame::getDebugImageDetections() / ...Matches(), drawn
// on the GPU when Params::debug_draw_detections / debug_draw_matches ask for them) to this object (which must outlive the Flame it feeds); `triangulate` stays empty, so the library's GPU Delaunay triangulation runs.  `track` hands every emitted feature of the frame
// to Flame (whose variance gate selects the ones that enter the graph) and fails the frame when fewer than three are emitted.
// Poses are T_world_cam; they cross into the library as row-major [R|t] in double, made from the unit quaternion and the
// translation of SE3f (Sophus::SE3f when present, the fallback struct otherwise).  Nothing throws; a failure leaves its code
// in lastError() (and the frame fails, which Flame reports like any failed update).
//
// RAW camera images: features.setCamera(raw_width, raw_height, resize_factor, D) before sensor.setFrontEnd(features.frontEnd())
// puts the library's ingest stage (integer downsample, plumb-bob undistortion; flame_hip.h, flame_hip_frontend_set_camera) in
// front of the tracker: update() then takes the grey image as the camera delivers it, raw_width x raw_height, and the K both
// objects were made with is the K of the rectified image (K_raw / resize_factor).  frontEnd() binds `rectified` as well, so the
// stages of Flame that read pixels (the evaluate stage) get the rectified image, downloaded once per frame and only when asked.
//
// GATES (flame_hip.h, flame_hip_frontend_set_gates; DESIGN.md 5.3 "Gates"): the constructor honours Params::do_letterbox
// (features only in the middle third of the rows) and Params::min_height / max_height (a tracked feature whose world point lies
// outside that band along the up axis is held back from the mesh); the height band is on iff min_height > -1e14f or max_height <
// 1e14f, so the reference's defaults set no gate and nothing changes.  setUpAxis() names the world's up direction (default
// (0, -1, 0): the reference's camera_world frame is right-down-forward [UPSTREAM-RECALL]); setGates() changes the gates later.  A
// record the library refuses (min_height > max_height, a zero or non-finite up axis, ...) leaves its code in lastError() and
// fails every track() until a valid one is set -- the gates are never dropped silently.
//
// MATCHING COST (flame_hip.h, flame_hip_frontend_set_cost; DESIGN.md 5.3 "Matching cost"): the constructor honours
// Params::zero_mean_matching (this build's own switch: the zero-mean SSD, bit-invariant to a grey offset between the pose frame
// and the current image); setZeroMean() changes it later, between any two frames.  With the switch off no call is made at all.  A
// refusal lands in lastError() and fails every track() until a call succeeds, as with the gates.  ZSSD does not remove a gain;
// Params::gain_invariant_matching (flame_hip_frontend_set_gain_invariant) does: the constructor honours it the same way -- off: no
// call at all --, setGainInvariant() changes it later, and while it is on it overrides the SSD / ZSSD choice.
//
// REFERENCE-PATCH GRADIENT (flame_hip.h, flame_hip_frontend_set_ref_grad; DESIGN.md 5.3 "Reference-patch gradient"): the constructor
// honours Params::min_epipolar_grad (this build's own switch: a feature whose reference window has no structure along its epipolar
// line is not searched); setRefGrad() changes it later, between any two frames.  With the switch at 0 no call is made at all and
// `num_fail_ref_patch_grad` stays unset.  A refusal (a negative or non-finite value) lands in lastError() and fails every track()
// until a call succeeds.
//
// WARPED WINDOW (flame_hip.h, flame_hip_frontend_set_warp; DESIGN.md 5.3 "Warped window"): the constructor honours
// Params::warp_matching_window (this build's own switch: the matching window follows the camera's roll and change of distance
// against the pose frame); setWarp() changes it later, between any two frames.  With the switch off no call is made at all and
// `num_fail_warp` stays unset.  A refusal lands in lastError() and fails every track() until a call succeeds.
//
// HAND-OVER (flame_hip.h, flame_hip_frontend_set_carry; DESIGN.md 5.3 "Hand-over"): the constructor honours Params::carry_features
// (this build's own switch: when a pose frame takes a ring slot in use, the features of the pose frame it evicts that the frame
// still emits are re-anchored in the new pose frame instead of dying); setCarry() changes it later, between any two frames.  With
// the switch off no call is made at all and `num_carried` / `num_carry_lost` stay unset.  A refusal lands in lastError() and fails
// every track() until a call succeeds.
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
    gates_.letterbox = params.do_letterbox ? 1 : 0;
    gates_.height_gate = (params.min_height > -1e14f || params.max_height < 1e14f) ? 1 : 0;
    gates_.min_height = params.min_height;
    gates_.max_height = params.max_height;
    gates_.up[0] = 0.f; gates_.up[1] = -1.f; gates_.up[2] = 0.f;
    if (handle_ && (gates_.letterbox || gates_.height_gate)) applyGates();  // (the reference's defaults: no call at all)
    if (handle_ && params.zero_mean_matching) {  // (off: no call at all)
      setZeroMean(true);
      if (gates_error_) last_error_ = gates_error_;  // (a refused gate record stays what lastError() shows)
    }
    if (handle_ && params.gain_invariant_matching) {  // (off: no call at all)
      const int before = last_error_;
      setGainInvariant(true);
      if (before) last_error_ = before;  // (an earlier refusal stays what lastError() shows)
    }
    if (handle_ && params.min_epipolar_grad != 0.f) {  // (off: no call at all)
      const int before = last_error_;
      setRefGrad(params.min_epipolar_grad);
      if (before) last_error_ = before;  // (an earlier refusal stays what lastError() shows)
    }
    if (handle_ && params.warp_matching_window) {  // (off: no call at all)
      const int before = last_error_;
      setWarp(true);
      if (before) last_error_ = before;  // (an earlier refusal stays what lastError() shows)
    }
    if (handle_ && params.carry_features) {  // (off: no call at all)
      const int before = last_error_;
      setCarry(true);
      if (before) last_error_ = before;  // (an earlier refusal stays what lastError() shows)
    }
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
    if (have_camera_) fe.rectified = [this]() { return rectified(); };
    fe.debugImage = [this](int kind, Image3b* out) { return debugImage(kind, out); };
    return fe;
  }

  // The ingest stage: raw GRAY8 images of raw_width x raw_height (update() takes an Image1b), downsampled by the integer
  // resize_factor to this object's width x height and undistorted with D = (k1, k2, p1, p2, k3) onto this object's K.  Call it
  // before frontEnd().  false (lastError()) when the library refuses the camera.
  bool setCamera(int raw_width, int raw_height, int resize_factor, const float D[5]) {
    if (!handle_) return false;
    flame_hip_camera cam;
    cam.raw_width = raw_width; cam.raw_height = raw_height; cam.format = FLAME_HIP_PIX_GRAY8; cam.resize_factor = resize_factor;
    for (int k = 0; k < 5; ++k) cam.D[k] = D[k];
    last_error_ = flame_hip_frontend_set_camera(handle_, &cam);
    have_camera_ = last_error_ == 0;
    if (have_camera_) { raw_width_ = raw_width; raw_height_ = raw_height; }
    return have_camera_;
  }
  bool hasCamera() const { return have_camera_; }

  // The gates of the frames to come.  setGates: the letterbox switch and the height band (height_gate = false: no band, the two
  // heights are not read); setUpAxis: the world direction heights are measured along (not normalised).  false (lastError()) when
  // the library refuses the record; track() then fails until a valid one is set.
  bool setGates(bool letterbox, bool height_gate, float min_height = -1e14f, float max_height = 1e14f) {
    gates_.letterbox = letterbox ? 1 : 0;
    gates_.height_gate = height_gate ? 1 : 0;
    gates_.min_height = min_height;
    gates_.max_height = max_height;
    return applyGates();
  }
  bool setUpAxis(float x, float y, float z) {
    gates_.up[0] = x; gates_.up[1] = y; gates_.up[2] = z;
    return applyGates();
  }
  const flame_hip_frontend_gates& gates() const { return gates_; }

  // The matching cost of the frames to come: the zero-mean SSD (true) or the plain SSD (false, the default).  May change between
  // any two frames: the feature state holds no cost.  false (lastError()) when the library refuses; track() then fails until a
  // call succeeds.
  bool setZeroMean(bool on) {
    if (!handle_) return false;
    cost_error_ = flame_hip_frontend_set_cost(handle_, on ? FLAME_HIP_FE_COST_ZSSD : FLAME_HIP_FE_COST_SSD);
    last_error_ = cost_error_;
    if (!cost_error_) zero_mean_ = on;
    return cost_error_ == 0;
  }
  bool zeroMean() const { return zero_mean_; }

  // The gain-invariant matching cost of the frames to come (true), which overrides the SSD / ZSSD choice while it is on, or that
  // choice again (false, the default).  May change between any two frames.  false (lastError()) when the library refuses; track()
  // then fails until a call succeeds.
  bool setGainInvariant(bool on) {
    if (!handle_) return false;
    gain_invariant_error_ = flame_hip_frontend_set_gain_invariant(handle_, on ? 1 : 0);
    last_error_ = gain_invariant_error_;
    if (!gain_invariant_error_) gain_invariant_ = on;
    return gain_invariant_error_ == 0;
  }
  bool gainInvariant() const { return gain_invariant_; }

  // The reference-patch gradient gate of the frames to come: the smallest root-mean-square grey gradient along the epipolar line a
  // reference window needs to be searched; 0 = off (the default).  May change between any two frames.  false (lastError()) when
  // the library refuses the value (negative, non-finite): the gate stays what it was and track() fails until a call succeeds.
  bool setRefGrad(float min_grad) {
    if (!handle_) return false;
    ref_grad_error_ = flame_hip_frontend_set_ref_grad(handle_, min_grad);
    last_error_ = ref_grad_error_;
    if (!ref_grad_error_) min_epipolar_grad_ = min_grad;
    return ref_grad_error_ == 0;
  }
  float refGrad() const { return min_epipolar_grad_; }

  // The warped matching window of the frames to come (true): the current image is sampled where the reference window's pixels land
  // under the pose change; false (the default): the axis-aligned window.  May change between any two frames.  false (lastError())
  // when the library refuses; track() then fails until a call succeeds.
  bool setWarp(bool on) {
    if (!handle_) return false;
    warp_error_ = flame_hip_frontend_set_warp(handle_, on ? 1 : 0);
    last_error_ = warp_error_;
    if (!warp_error_) warp_ = on;
    return warp_error_ == 0;
  }
  bool warp() const { return warp_; }

  // The hand-over of the pose frames to come (true): a pose frame that takes a ring slot in use re-anchors the evicted pose frame's
  // features that it emits in itself, the others die behind the frame; false (the default): they all die before it.  May change
  // between any two frames.  false (lastError()) when the library refuses; track() then fails until a call succeeds.
  bool setCarry(bool on) {
    if (!handle_) return false;
    carry_error_ = flame_hip_frontend_set_carry(handle_, on ? 1 : 0);
    last_error_ = carry_error_;
    if (!carry_error_) carry_ = on;
    return carry_error_ == 0;
  }
  bool carry() const { return carry_; }

  // The ingest stage alone (flame_hip_frontend_rectify): `out` becomes the width x height rectified image of `raw`; the
  // feature state is untouched.
  bool rectify(const Image1b& raw, Image1b* out) {
    if (!handle_) return false;
    if (!have_camera_) return fail(FLAME_HIP_ERR_STATE);
    if (!out || raw.rows != raw_height_ || raw.cols != raw_width_) return fail(FLAME_HIP_ERR_ARG);
    if (out->rows != height_ || out->cols != width_) *out = Image1b(height_, width_);
    const int rc = flame_hip_frontend_rectify(handle_, raw.ptr<uint8_t>(0), pitchOf(raw), out->ptr<uint8_t>(0), pitchOf(*out));
    if (rc) return fail(rc);
    last_error_ = 0;
    return true;
  }

  // The image the last track() tracked (after the ingest stage), downloaded on the first call after that track(); nullptr
  // (lastError()) when there is none.
  const Image1b* rectified() {
    if (!handle_) return nullptr;
    if (!rectified_valid_) {
      if (rectified_.rows != height_ || rectified_.cols != width_) rectified_ = Image1b(height_, width_);
      const int rc = flame_hip_frontend_image(handle_, rectified_.ptr<uint8_t>(0), pitchOf(rectified_));
      if (rc) { last_error_ = rc; return nullptr; }
      rectified_valid_ = true;
    }
    return &rectified_;
  }

  // The Detections / Matches debug image (FLAME_HIP_FE_IMG_*; flame_hip.h, flame_hip_frontend_debug_image) of the last frame
  // track() tracked, rendered on the GPU: `*out` becomes width x height BGR8.  false (lastError()) before the first frame.
  bool debugImage(int kind, Image3b* out) {
    if (!handle_) return false;
    if (!out) return fail(FLAME_HIP_ERR_ARG);
    if (out->rows != height_ || out->cols != width_) *out = Image3b(height_, width_);
    static_assert(sizeof(Vec3b) == 3, "BGR8 pixels are packed");
    const int32_t pitch = height_ > 1 ? static_cast<int32_t>(out->ptr<uint8_t>(1) - out->ptr<uint8_t>(0)) : 3 * width_;
    const int rc = flame_hip_frontend_debug_image(handle_, kind, out->ptr<uint8_t>(0), pitch);
    if (rc) return fail(rc);
    return true;
  }

  bool track(const FrameInput& in, FeatureSet* out) {
    if (!handle_) return false;  // (lastError() still holds why the handle could not be made)
    if (gates_error_) return fail(gates_error_);  // (a refused gate record is not tracked around)
    if (cost_error_) return fail(cost_error_);    // (nor a refused matching cost)
    if (gain_invariant_error_) return fail(gain_invariant_error_);
    if (ref_grad_error_) return fail(ref_grad_error_);  // (nor a refused gradient gate)
    if (warp_error_) return fail(warp_error_);          // (nor a refused warp switch)
    if (carry_error_) return fail(carry_error_);        // (nor a refused hand-over switch)
    rectified_valid_ = false;
    const int rows = have_camera_ ? raw_height_ : height_, cols = have_camera_ ? raw_width_ : width_;
    if (!in.img || !out || in.img->rows != rows || in.img->cols != cols) return fail(FLAME_HIP_ERR_ARG);
    double T[12];
    toRt(in.pose, T);
    const uint8_t* row0 = in.img->ptr<uint8_t>(0);
    const int32_t pitch = pitchOf(*in.img);
    int32_t n = 0;
    int rc = have_camera_ ? flame_hip_frontend_track_raw(handle_, &fparams_, row0, pitch, in.img_id, T, in.is_poseframe ? 1 : 0, &n)
                          : flame_hip_frontend_track(handle_, &fparams_, row0, pitch, in.img_id, T, in.is_poseframe ? 1 : 0, &n);
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
  // matches above the cost threshold.  `num_fail_max_var` is Flame's own (its variance gate); `num_fail_ref_patch_grad` is
  // the features the reference-patch gradient gate refused and is set only while that gate is on (it is off by default: unset);
  // `num_fail_warp` is the features the warped window refused and is set only while that switch is on; `num_carried` and
  // `num_carry_lost` are the evicted pose frame's features the frame handed over / lost and are set only while the hand-over is on.
  void reportStats(utils::StatsTracker* stats) const {
    if (!handle_ || !stats) return;
    static const char* const kKeys[4][2] = {{"num_idepth_updates", "ok"}, {"num_fail_max_dropouts", "died"},
                                            {"num_fail_ambiguous_match", "ambiguous"}, {"num_fail_max_cost", "bad_match"}};
    for (int k = 0; k < 4; ++k) {
      int64_t v = 0;
      if (flame_hip_frontend_info(handle_, kKeys[k][1], &v) == 0) stats->set(kKeys[k][0], static_cast<double>(v));
    }
    // this build's own keys, with a gate on only: features the height band held, projections the letterbox refused
    int64_t g = 0, v = 0;
    if (flame_hip_frontend_info(handle_, "gates", &g) == 0 && g != 0) {
      if (flame_hip_frontend_info(handle_, "held_height", &v) == 0) stats->set("num_held_height", static_cast<double>(v));
      if (flame_hip_frontend_info(handle_, "refused_letterbox", &v) == 0) stats->set("num_refused_letterbox", static_cast<double>(v));
    }
    if (flame_hip_frontend_info(handle_, "ref_grad", &g) == 0 && g != 0) {
      if (flame_hip_frontend_info(handle_, "fail_ref_grad", &v) == 0) stats->set("num_fail_ref_patch_grad", static_cast<double>(v));
    }
    if (flame_hip_frontend_info(handle_, "warp", &g) == 0 && g != 0) {
      if (flame_hip_frontend_info(handle_, "warp_refused", &v) == 0) stats->set("num_fail_warp", static_cast<double>(v));
    }
    if (flame_hip_frontend_info(handle_, "carry", &g) == 0 && g != 0) {
      if (flame_hip_frontend_info(handle_, "carried", &v) == 0) stats->set("num_carried", static_cast<double>(v));
      if (flame_hip_frontend_info(handle_, "carry_lost", &v) == 0) stats->set("num_carry_lost", static_cast<double>(v));
    }
  }

  // [R|t], row-major 3x4 in double (flame/types.h poseToRt, shared with Flame's prediction stage)
  static void toRt(const SE3f& pose, double T[12]) { poseToRt(pose, T); }

 private:
  bool fail(int code) {
    last_error_ = code;
    return false;
  }
  bool applyGates() {
    if (!handle_) return false;
    gates_error_ = flame_hip_frontend_set_gates(handle_, (gates_.letterbox || gates_.height_gate) ? &gates_ : nullptr);
    last_error_ = gates_error_;
    return gates_error_ == 0;
  }
  static int32_t pitchOf(const Image1b& img) {
    return img.rows > 1 ? static_cast<int32_t>(img.ptr<uint8_t>(1) - img.ptr<uint8_t>(0)) : img.cols;
  }
  int width_, height_;
  bool have_camera_ = false;
  int raw_width_ = 0, raw_height_ = 0;
  Image1b rectified_;             // the image of the last track(), downloaded on demand
  bool rectified_valid_ = false;
  flame_hip_frontend_params fparams_;
  flame_hip_frontend_gates gates_;
  int gates_error_ = 0;  // what the library said to the last gate record
  bool zero_mean_ = false;
  int cost_error_ = 0;   // ... and to the last matching cost
  bool gain_invariant_ = false;
  int gain_invariant_error_ = 0;  // ... and to the last gain-invariant switch
  float min_epipolar_grad_ = 0.f;
  int ref_grad_error_ = 0;  // ... and to the last gradient gate
  bool warp_ = false;
  int warp_error_ = 0;      // ... and to the last warp switch
  bool carry_ = false;
  int carry_error_ = 0;     // ... and to the last hand-over switch
  flame_hip_frontend* handle_ = nullptr;
  int last_error_ = 0;
};

}  // namespace flame
