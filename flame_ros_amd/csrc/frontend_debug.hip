// flame_ros_amd/csrc/frontend_debug.hip -- the feature front end's two debug images (gfx950), rendered on demand from the record
// the last tracked frame left on the device: Matches (every epipolar search as the tracker sampled it, green = OK, red = failed,
// yellow = the best sample of an OK search) and Detections (a 3 x 3 square per emitted feature, green = NEW, blue = tracked), both
// over the tracked grey image.  The statement: DESIGN.md 5.3 "Debug images"; tests/fe_debug_ref.py restates it and the GPU equals
// it byte for byte.
//
// The result is an integer picture whose colour depends on the LAYER alone, so one launch per layer in stream order, each storing
// one constant colour, gives the same bytes whatever order slots, samples and lanes arrive in: two lanes that meet on a pixel
// within a launch store the same three bytes.  No atomics, no LDS.  Sample positions are the tracker's own expression
// x0 + (float)k * ex (float32, no fused multiply-add: -ffp-contract=off), from the very {x0, y0, ex, ey} it searched with.
//
// Memory: the picture is dense BGR8 (3 W bytes a row, 256-byte aligned base): the background is written as packed dwords, four
// pixels a thread; samples and squares are byte stores (<= 1 MB, stays in L2).  The grey image is read by bytes (a ring slot
// starts at any address).
#include "frontend.h"

namespace flamehip {

namespace {

// four pixels a thread: 4 grey bytes in, 12 BGR bytes (3 dwords) out; the last thread finishes by bytes
__global__ __launch_bounds__(256) void k_fd_background(const uint8_t* __restrict__ grey, uint8_t* __restrict__ bgr, int npix) {
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= npix) return;
  if (i + 3 < npix) {
    const unsigned int a = grey[i], b = grey[i + 1], c = grey[i + 2], d = grey[i + 3];
    unsigned int* __restrict__ o = reinterpret_cast<unsigned int*>(bgr + (size_t)3 * i);  // (12 i bytes from an aligned base)
    o[0] = a | (a << 8) | (a << 16) | (b << 24);
    o[1] = b | (b << 8) | (c << 16) | (c << 24);
    o[2] = c | (d << 8) | (d << 16) | (d << 24);
  } else {
    for (int j = i; j < npix; ++j) {
      const uint8_t g = grey[j];
      bgr[(size_t)3 * j] = g;
      bgr[(size_t)3 * j + 1] = g;
      bgr[(size_t)3 * j + 2] = g;
    }
  }
}

__device__ __forceinline__ void fd_put(const FeFrame& f, uint8_t* __restrict__ bgr, float px, float py, uint8_t b, uint8_t g, uint8_t r) {
  const float X = floorf(px + 0.5f), Y = floorf(py + 0.5f);
  if (!(X >= 0.0f && X <= (float)(f.W - 1) && Y >= 0.0f && Y <= (float)(f.H - 1))) return;  // (a NaN or infinite position fails too)
  uint8_t* __restrict__ o = bgr + ((size_t)(int)Y * f.W + (int)X) * 3;
  o[0] = b;
  o[1] = g;
  o[2] = r;
}

// One wavefront per slot, lanes over the samples lane + 64 pass (the tracker's shape).  layer 1: the samples of OK slots, green;
// layer 2: the samples of OUTSIDE / BAD_MATCH / AMBIGUOUS / DIED slots, red; layer 3: sample k* of OK slots, yellow.
__global__ __launch_bounds__(256) void k_fd_matches(FeFrame f, uint8_t* __restrict__ bgr, int layer) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= f.max_features) return;
  const int S = f.steps[slot], st = f.status[slot];
  if (S <= 0 || S > kFeMaxSamples) return;
  const bool ok = st == kFeOk;
  const bool red = st == kFeOutside || st == kFeBadMatch || st == kFeAmbiguous || st == kFeDied;
  if (layer == 2 ? !red : !ok) return;
  const float4 sg = f.seg[slot];
  if (layer == 3) {
    const int ks = f.kstar[slot];
    if (lane == 0 && ks >= 0 && ks <= S) fd_put(f, bgr, sg.x + (float)ks * sg.z, sg.y + (float)ks * sg.w, 0, 255, 255);
    return;
  }
  const uint8_t g = layer == 1 ? 255 : 0, r = layer == 1 ? 0 : 255;
#pragma unroll
  for (int pass = 0; pass < kFePasses; ++pass) {
    const int k = lane + 64 * pass;
    if (k <= S) fd_put(f, bgr, sg.x + (float)k * sg.z, sg.y + (float)k * sg.w, 0, g, r);
  }
}

// One thread per emitted record: its 3 x 3 square, clipped.  layer 1: every feature that is not NEW, blue; layer 2: NEW, green.
__global__ __launch_bounds__(256) void k_fd_detections(FeFrame f, int n_out, uint8_t* __restrict__ bgr, int layer) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_out) return;
  const FeOut o = f.out[i];
  if ((o.status == kFeNew) != (layer == 2)) return;
  const float X = floorf(o.x + 0.5f), Y = floorf(o.y + 0.5f);
  if (!(X >= -1.0f && X <= (float)f.W && Y >= -1.0f && Y <= (float)f.H)) return;  // no pixel of the square is inside (or NaN)
  const int cx = (int)X, cy = (int)Y;
  const uint8_t b = layer == 2 ? 0 : 255, g = layer == 2 ? 255 : 0;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int x = cx + dx, y = cy + dy;
      if (x < 0 || x > f.W - 1 || y < 0 || y > f.H - 1) continue;
      uint8_t* __restrict__ q = bgr + ((size_t)y * f.W + x) * 3;
      q[0] = b;
      q[1] = g;
      q[2] = 0;
    }
}

void fd_background(hipStream_t s, const FeFrame& f, uint8_t* bgr) {
  const int npix = f.W * f.H;
  hipLaunchKernelGGL(k_fd_background, dim3((npix + 1023) / 1024), dim3(256), 0, s, f.cur, bgr, npix);
}

}  // namespace

void fe_launch_debug_matches(hipStream_t s, const FeFrame& f, uint8_t* bgr) {
  fd_background(s, f, bgr);
  for (int layer = 1; layer <= 3; ++layer)
    hipLaunchKernelGGL(k_fd_matches, dim3((f.max_features + 3) / 4), dim3(256), 0, s, f, bgr, layer);
}

void fe_launch_debug_detections(hipStream_t s, const FeFrame& f, int32_t n_out, uint8_t* bgr) {
  fd_background(s, f, bgr);
  if (n_out <= 0) return;
  for (int layer = 1; layer <= 2; ++layer)
    hipLaunchKernelGGL(k_fd_detections, dim3((n_out + 255) / 256), dim3(256), 0, s, f, n_out, bgr, layer);
}

}  // namespace flamehip
