// flame_ros_amd/csrc/ingest.hip -- kernels of the ingest stage (gfx950): grey conversion + integer box downsample
// (k_in_grey_box) and plumb-bob undistortion onto the same camera matrix (k_in_remap).
//
// Arithmetic contract: the grey and box steps are integers; the remap is float32 with + - x / floorf only,
// every operation rounded on its own (-ffp-contract=off, NO fmaf), products and sums left to right exactly as distortPoint()
// and undistort<uint8_t>() of include/flame_ros/image_io.h write them.  tests/ingest_ref.py restates both in NumPy and the
// GPU must equal it bit for bit.  Every step is rounded to uint8, so running the steps as one kernel or two gives the same bits.
//
// Work distribution: one output pixel per lane, workgroups of 64 x 4 pixels -- the 64 lanes of a wavefront lie along an image
// row, so a wavefront's store is 64 consecutive bytes and its four gather taps fall on two short runs of two source rows.
// Rows are dense W bytes at any address: every access is a byte access (a 752 x 480 source is 361 KB and stays in L2).
#include "ingest.h"

namespace flamehip {

namespace {

constexpr int kInBx = 64, kInBy = 4;

__device__ __forceinline__ int in_grey(const uint8_t* __restrict__ p, int format) {
  if (format == kInGray8) return p[0];
  const int c0 = p[0], g = p[1], c2 = p[2];
  const int r = (format == kInBgr8 || format == kInBgra8) ? c2 : c0;
  const int b = (format == kInBgr8 || format == kInBgra8) ? c0 : c2;
  return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14;
}

__global__ __launch_bounds__(kInBx * kInBy) void k_in_grey_box(InCam c, const uint8_t* __restrict__ raw, int raw_pitch,
                                                                uint8_t* __restrict__ out) {
  const int x = blockIdx.x * kInBx + threadIdx.x, y = blockIdx.y * kInBy + threadIdx.y;
  if (x >= c.W || y >= c.H) return;
  const int f = c.f, ch = c.format == kInGray8 ? 1 : (c.format == kInBgr8 || c.format == kInRgb8) ? 3 : 4;
  int sum = 0;  // <= 64 * 255
  for (int dy = 0; dy < f; ++dy) {
    const uint8_t* __restrict__ row = raw + (size_t)(f * y + dy) * raw_pitch + (size_t)(f * x) * ch;
    for (int dx = 0; dx < f; ++dx) sum += in_grey(row + dx * ch, c.format);
  }
  out[(size_t)y * c.W + x] = (uint8_t)((sum + ((f * f) >> 1)) / (f * f));
}

__global__ __launch_bounds__(kInBx * kInBy) void k_in_remap(InCam c, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
  const int u = blockIdx.x * kInBx + threadIdx.x, v = blockIdx.y * kInBy + threadIdx.y;
  if (u >= c.W || v >= c.H) return;
  const int W = c.W, H = c.H;
  // distortPoint()
  const float x = ((float)u - c.cx) / c.fx, y = ((float)v - c.cy) / c.fy;
  const float r2 = x * x + y * y;
  const float radial = 1.0f + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3));
  const float xd = x * radial + 2.0f * c.p1 * x * y + c.p2 * (r2 + 2.0f * x * x);
  const float yd = y * radial + c.p1 * (r2 + 2.0f * y * y) + 2.0f * c.p2 * x * y;
  const float su = c.fx * xd + c.cx, sv = c.fy * yd + c.cy;
  uint8_t o = 0;
  // (tested in float before any conversion to int: a NaN or infinite source position fails it)
  if (su > -1.0f && su < (float)W && sv > -1.0f && sv < (float)H) {
    // undistort<uint8_t>(): bilinear, taps outside the image read 0
    const float fx0 = floorf(su), fy0 = floorf(sv);
    const int x0 = (int)fx0, y0 = (int)fy0;  // in [-1, W - 1] x [-1, H - 1]
    const float ax = su - fx0, ay = sv - fy0;
    const bool xl = x0 >= 0, xr = x0 + 1 < W, yt = y0 >= 0, yb = y0 + 1 < H;
    const uint8_t* __restrict__ p = src + (ptrdiff_t)y0 * W + x0;
    const float a00 = (xl && yt) ? (float)p[0] : 0.0f;
    const float a10 = (xr && yt) ? (float)p[1] : 0.0f;
    const float a01 = (xl && yb) ? (float)p[W] : 0.0f;
    const float a11 = (xr && yb) ? (float)p[W + 1] : 0.0f;
    const float top = a00 + ax * (a10 - a00);
    const float bot = a01 + ax * (a11 - a01);
    const float val = top + ay * (bot - top);
    o = (uint8_t)(val + 0.5f);
  }
  dst[(size_t)v * W + u] = o;
}

inline dim3 in_grid(const InCam& c) { return dim3((c.W + kInBx - 1) / kInBx, (c.H + kInBy - 1) / kInBy); }

}  // namespace

void in_launch_grey_box(hipStream_t s, const InCam& c, const uint8_t* raw, int32_t raw_pitch, uint8_t* out) {
  hipLaunchKernelGGL(k_in_grey_box, in_grid(c), dim3(kInBx, kInBy), 0, s, c, raw, raw_pitch, out);
}
void in_launch_remap(hipStream_t s, const InCam& c, const uint8_t* src, uint8_t* dst) {
  hipLaunchKernelGGL(k_in_remap, in_grid(c), dim3(kInBx, kInBy), 0, s, c, src, dst);
}

}  // namespace flamehip
