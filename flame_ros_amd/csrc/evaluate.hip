// flame_ros_amd/csrc/evaluate.hip -- kernels of the evaluate stage (evaluate.h) for gfx950.
//
// Arithmetic contract (the one of DESIGN.md 5.3 / 5.4): float32 with + - x / floorf only, every operation rounded on its own
// (-ffp-contract=off, and NO fmaf anywhere in this file); sums run left to right as written.  The photometric costs are
// integers, so any reduction order gives the same bits; there are no floating-point atomics.  tests/eval_ref.py restates
// every expression below in NumPy and the GPU equals it bit for bit, so an expression here is changed together with its twin
// there or not at all.
//
// Both kernels: 256 threads per block, block b owns pixels [1024 b, 1024 (b + 1)), thread t the pixels 1024 b + 256 r + t,
// r = 0 .. 3.  Lanes accumulate in registers, a wave reduction follows (shuffles for the sums, ballot + popcount for the
// counts), the four waves meet in LDS, and one 64-bit integer atomicAdd per word and block lands in the handle's words.
#include <hip/hip_runtime.h>

#include "evaluate.h"

namespace flamehip {
namespace {

__device__ __forceinline__ bool ev_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }
__device__ __forceinline__ bool ev_isnan(float x) { return x != x; }

// q = floorf(p x 16 + 0.5f) of one axis of n pixels: admissible when the integer part q >> 4 lies in [0, n - 2] (the +1
// bilinear neighbour is inside); compared in float, so a huge or NaN pixel never reaches the integer conversion
__device__ __forceinline__ bool ev_sixteenths(float p, int32_t n, int& q) {
  const float fq = floorf(p * 16.0f + 0.5f);
  if (!(fq >= 0.0f && fq < (float)(16 * (n - 1)))) return false;
  q = (int)fq;
  return true;
}

__global__ __launch_bounds__(256) void k_ev_photo(EvPhoto f) {
  __shared__ unsigned long long s_part[4][kEvPhotoWords];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t npix = (int64_t)f.W * f.H;
  const float* A = f.pose.A;
  uint32_t dsum = 0;                  // <= 4 x 65 280 per lane
  uint32_t cnt[4] = {0u, 0u, 0u, 0u}; // wave-uniform: evaluated, no_idepth, behind, outside
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t k = (int64_t)blockIdx.x * kEvBlockPixels + r * 256 + (int)threadIdx.x;
    int cls = -1;
    uint32_t D = 0;
    if (k < npix) {
      const int i = (int)(k / f.W), j = (int)(k - (int64_t)i * f.W);
      const float xi = f.idepth[k];
      if (!(ev_finite(xi) && xi > 0.0f)) {
        cls = kEvNoIdepth;
      } else {
        const float b0 = ((float)j - f.cx) / f.fx, b1 = ((float)i - f.cy) / f.fy;
        const float w0 = ((A[0] * b0 + A[1] * b1) + A[2]) + xi * f.pose.c[0];
        const float w1 = ((A[3] * b0 + A[4] * b1) + A[5]) + xi * f.pose.c[1];
        const float w2 = ((A[6] * b0 + A[7] * b1) + A[8]) + xi * f.pose.c[2];
        int qx = 0, qy = 0;
        if (!(w2 > 0.0f) || !ev_finite(w0) || !ev_finite(w1) || !ev_finite(w2)) {
          cls = kEvBehind;
        } else if (!ev_sixteenths(w0 / w2, f.W, qx) || !ev_sixteenths(w1 / w2, f.H, qy)) {
          cls = kEvOutside;
        } else {
          const int ix = qx >> 4, iy = qy >> 4;  // 0 <= ix <= W - 2, 0 <= iy <= H - 2
          const uint32_t wx1 = (uint32_t)(qx & 15), wx0 = 16u - wx1, wy1 = (uint32_t)(qy & 15), wy0 = 16u - wy1;
          const uint8_t* __restrict__ r0 = f.cmp + (size_t)iy * f.W + ix;
          const uint8_t* __restrict__ r1 = r0 + f.W;
          const uint32_t S = (wx0 * wy0 * r0[0] + wx1 * wy0 * r0[1]) + (wx0 * wy1 * r1[0] + wx1 * wy1 * r1[1]);
          const uint32_t C = 256u * f.cur[k];
          D = S > C ? S - C : C - S;
          cls = kEvEvaluated;
        }
      }
      if (f.err) f.err[k] = cls == kEvEvaluated ? (float)D / 256.0f : __builtin_nanf("");
    }
    dsum += D;
    cnt[0] += (uint32_t)__popcll(__ballot(cls == kEvEvaluated));
    cnt[1] += (uint32_t)__popcll(__ballot(cls == kEvNoIdepth));
    cnt[2] += (uint32_t)__popcll(__ballot(cls == kEvBehind));
    cnt[3] += (uint32_t)__popcll(__ballot(cls == kEvOutside));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dsum += __shfl_xor(dsum, o, 64);  // <= 64 x 261 120: no overflow
  if (lane == 0) {
    s_part[wv][kEvTotal256] = dsum;
    s_part[wv][kEvEvaluated] = cnt[0];
    s_part[wv][kEvNoIdepth] = cnt[1];
    s_part[wv][kEvBehind] = cnt[2];
    s_part[wv][kEvOutside] = cnt[3];
  }
  __syncthreads();
  if (threadIdx.x < kEvPhotoWords) {
    const unsigned long long v = (s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + (s_part[2][threadIdx.x] + s_part[3][threadIdx.x]);
    if (v != 0ull) atomicAdd(f.words + threadIdx.x, v);
  }
}

// The loop of reference src/utils.cc:339-365, its branches in its order.
__global__ __launch_bounds__(256) void k_ev_truth(EvTruth f) {
  __shared__ double s_sum[4];
  __shared__ uint32_t s_cnt[4][kEvTruthWords];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double v = 0.0;
  uint32_t cnt[4] = {0u, 0u, 0u, 0u};  // wave-uniform: true_pos, true_neg, false_pos, false_neg
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t k = (int64_t)blockIdx.x * kEvBlockPixels + r * 256 + (int)threadIdx.x;
    int cls = -1;
    float e = 0.0f;  // (a pixel without an error adds +0.0: the tree's shape does not depend on the data)
    if (k < f.npix) {
      const float depth = f.depth[k], est = f.idepth[k];
      if (depth > 0.0f) {
        if (!ev_isnan(est)) {
          const float idepth_true = 1.0f / depth;
          e = __builtin_fabsf(est - idepth_true);
          cls = kEvTruePos;
        } else {
          cls = kEvFalseNeg;
        }
      } else if (!ev_isnan(est)) {
        e = __builtin_fabsf(est);
        cls = kEvFalsePos;
      } else {
        cls = kEvTrueNeg;
      }
      if (f.err) f.err[k] = (cls == kEvTruePos || cls == kEvFalsePos) ? e : __builtin_nanf("");
    }
    v = v + (double)e;
    cnt[0] += (uint32_t)__popcll(__ballot(cls == kEvTruePos));
    cnt[1] += (uint32_t)__popcll(__ballot(cls == kEvTrueNeg));
    cnt[2] += (uint32_t)__popcll(__ballot(cls == kEvFalsePos));
    cnt[3] += (uint32_t)__popcll(__ballot(cls == kEvFalseNeg));
  }
  // the fixed tree: lane l takes lane l + o for o = 32, 16, .. 1 (lane 0 holds the wave's sum), then ((w0 + w1) + w2) + w3
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_down(v, o, 64);
  if (lane == 0) {
    s_sum[wv] = v;
#pragma unroll
    for (int c = 0; c < kEvTruthWords; ++c) s_cnt[wv][c] = cnt[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) f.partial[blockIdx.x] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
  if (threadIdx.x < kEvTruthWords) {
    const unsigned long long n = (unsigned long long)s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
    if (n != 0ull) atomicAdd(f.words + threadIdx.x, n);
  }
}

}  // namespace

void ev_launch_photo(hipStream_t s, const EvPhoto& f) {
  const int64_t npix = (int64_t)f.W * f.H;
  if (npix > 0) hipLaunchKernelGGL(k_ev_photo, dim3((unsigned)ev_num_blocks(npix)), dim3(256), 0, s, f);
}

void ev_launch_truth(hipStream_t s, const EvTruth& f) {
  if (f.npix > 0) hipLaunchKernelGGL(k_ev_truth, dim3((unsigned)ev_num_blocks(f.npix)), dim3(256), 0, s, f);
}

}  // namespace flamehip
