// flame_ros_amd/csrc/ingest.h -- the ingest stage in front of the feature front end: a raw camera image (grey or colour, any
// integer resize factor, plumb-bob distortion) becomes the rectified grey image the tracker reads.  Kernels: ingest.hip; C ABI:
// frontend.cpp (include/flame_hip.h, flame_hip_frontend_set_camera / _track_raw / _rectify); the statement: DESIGN.md 5.6.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flamehip {

// pixel formats (FLAME_HIP_PIX_* of include/flame_hip.h)
enum { kInGray8 = 0, kInBgr8 = 1, kInRgb8 = 2, kInBgra8 = 3, kInRgba8 = 4, kInFormats = 5 };
constexpr int kInMaxResize = 8;

inline int in_channels(int format) { return format == kInGray8 ? 1 : (format == kInBgr8 || format == kInRgb8) ? 3 : 4; }

// the camera of a handle: raw geometry, and K / D of the OUTPUT image (W = raw_w / f, H = raw_h / f)
struct InCam {
  int32_t raw_w, raw_h, format, f, W, H;
  float fx, fy, cx, cy;
  float k1, k2, p1, p2, k3;
};

// grey + box: raw (rows raw_pitch bytes apart, in_channels(format) bytes per pixel) -> W x H dense grey
void in_launch_grey_box(hipStream_t s, const InCam& c, const uint8_t* raw, int32_t raw_pitch, uint8_t* out);
// remap: W x H dense grey (distorted) -> W x H dense grey (undistorted onto the same K)
void in_launch_remap(hipStream_t s, const InCam& c, const uint8_t* src, uint8_t* dst);

}  // namespace flamehip
