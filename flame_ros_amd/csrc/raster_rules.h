// flame_ros_amd/csrc/raster_rules.h -- rules of the dense raster that more than one file states pixels by (kernels.hip: the
// owner pass of the dense maps; predict.hip: the z-buffer of the prediction stage).
#pragma once
#include <hip/hip_runtime.h>

namespace flamehip {

// The bounding box along one axis of n pixels: clamped to [-1, n] in float before the conversion to int
// (a vertex beyond 2^31 px must not reach the conversion; oracle raster_span), then to the image.
__device__ __forceinline__ void raster_span(float lo, float hi, int n, int& i0, int& i1) {
  i0 = max((int)ceilf(fminf(fmaxf(lo, -1.0f), (float)n)), 0);
  i1 = min((int)floorf(fminf(fmaxf(hi, -1.0f), (float)n)), n - 1);
}

}  // namespace flamehip
