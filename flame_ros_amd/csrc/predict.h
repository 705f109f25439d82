// flame_ros_amd/csrc/predict.h -- the prediction stage (upstream's project_graph): the previous frame's regularised,
// validity-filtered mesh warped into the current camera view and z-buffered; an inverse-depth prediction per query pixel and a
// dense predicted idepth map are read from it.  Kernels: predict.hip; C ABI: flame_hip_predict / flame_hip_predict_map
// (flame_hip.cpp); the statement: DESIGN.md 5.4, restated operation by operation in tests/predict_ref.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frontend.h"

namespace flamehip {

struct PgFrame {
  int32_t V, T, W, H, n;
  float fx, fy, cx, cy;
  FePose pose;            // A = K R, c = K t of T_cur_prev (frontend.h pose_record)
  // the previous frame as the handle holds it (internal vertex ids, the caller's triangle order)
  const float2* pos;      // V vertex pixels
  const float4* A;        // V, .x = idepth in the caller's units
  const int32_t* tris;    // 3 T
  const uint8_t* tri_valid;
  // the stage's own buffers
  float4* proj;                 // V: {warped pixel x, y, idepth in the current frame, ok (1 / 0)}
  unsigned long long* key;      // W x H: max over covering triangles of (bits(idepth) << 32 | 0xFFFFFFFF - t); 0 = empty
  const float2* pix;            // n query pixels
  float* pred;                  // n
};

// (the map's clear is a memset the caller queues in front of these)
void pg_launch_project(hipStream_t s, const PgFrame& f);
void pg_launch_zbuffer(hipStream_t s, const PgFrame& f);
void pg_launch_sample(hipStream_t s, const PgFrame& f);
// dense map: the high word of a non-empty key as float, NaN where empty
void pg_launch_map(hipStream_t s, int64_t npix, const unsigned long long* key, float* map);

}  // namespace flamehip
