// flame_ros_amd/csrc/predict.hip -- kernels of the prediction stage (predict.h) for gfx950.
//
// Arithmetic contract: float32 with + - x / floorf ceilf only, every operation rounded on its own (-ffp-contract=off, and NO
// fmaf anywhere in this file); sums run left to right as written.  tests/predict_ref.py restates every expression below in
// NumPy and the GPU equals it bit for bit, so an expression here is changed together with its twin there or not at all.
//
// Three launches behind the key map's clear: k_pg_project (one thread per previous vertex), k_pg_zbuffer (the dense raster's
// lanes-per-triangle scheme, kernels.hip raster_owner_body: 64 lanes per triangle for meshes of large triangles, 8 for dense
// ones with the whole wave for boxes above 256 pixels), k_pg_sample (one thread per query).  The key map is a maximum of
// 64-bit keys -- the pattern of frontend.hip's cell_key --, hence a function of the inputs alone in any execution order.
#include <hip/hip_runtime.h>

#include "predict.h"
#include "raster_rules.h"

namespace flamehip {
namespace {

__device__ __forceinline__ bool pg_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }

// e(a, b, p) = (bx - ax) (py - ay) - (by - ay) (px - ax)
__device__ __forceinline__ float pg_e(float ax, float ay, float bx, float by, float px, float py) {
  return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

// The dense raster's watertight rule (kernels.hip edge_w) on e(): an edge is evaluated from its lexicographically smaller end
// point, so the two triangles of a shared edge see exactly opposite values.
__device__ __forceinline__ float pg_edge_w(float ax, float ay, float bx, float by, float px, float py) {
  const bool a_first = ax < bx || (ax == bx && ay < by);
  return a_first ? pg_e(ax, ay, bx, by, px, py) : -pg_e(bx, by, ax, ay, px, py);
}

// weights of (px, py) in the warped triangle (a, b, c) and the interpolated idepth; `in` = all weights >= 0 or all <= 0
__device__ __forceinline__ float pg_interp(float4 a, float4 b, float4 c, float px, float py, bool& in) {
  const float wa = pg_edge_w(b.x, b.y, c.x, c.y, px, py);
  const float wb = pg_edge_w(c.x, c.y, a.x, a.y, px, py);
  const float wc = pg_edge_w(a.x, a.y, b.x, b.y, px, py);
  in = (wa >= 0.f && wb >= 0.f && wc >= 0.f) || (wa <= 0.f && wb <= 0.f && wc <= 0.f);
  return ((wa * a.z + wb * b.z) + wc * c.z) / ((wa + wb) + wc);
}

__global__ __launch_bounds__(256) void k_pg_project(PgFrame f) {
  const int v = (int)(blockIdx.x * 256 + threadIdx.x);
  if (v >= f.V) return;
  const float2 p = f.pos[v];
  const float x = f.A[v].x;
  const float b0 = (p.x - f.cx) / f.fx, b1 = (p.y - f.cy) / f.fy;
  const float* A = f.pose.A;
  const float w0 = ((A[0] * b0 + A[1] * b1) + A[2]) + x * f.pose.c[0];
  const float w1 = ((A[3] * b0 + A[4] * b1) + A[5]) + x * f.pose.c[1];
  const float w2 = ((A[6] * b0 + A[7] * b1) + A[8]) + x * f.pose.c[2];
  const bool ok = pg_finite(x) && x > 0.f && w2 > 0.f && pg_finite(w0) && pg_finite(w1) && pg_finite(w2);
  f.proj[v] = ok ? make_float4(w0 / w2, w1 / w2, x / w2, 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ void pg_cover(float4 a, float4 b, float4 c, int x0, int y0, int bw, int n, int first, int step,
                                         int32_t width, uint32_t t, unsigned long long* __restrict__ key) {
  for (int k = first; k < n; k += step) {
    const int jj = x0 + k % bw, ii = y0 + k / bw;
    bool in;
    const float xi = pg_interp(a, b, c, (float)jj, (float)ii, in);
    if (in && pg_finite(xi) && xi > 0.f)
      atomicMax(key + (size_t)ii * width + jj, ((unsigned long long)__float_as_uint(xi) << 32) | (unsigned long long)(0xFFFFFFFFu - t));
  }
}

template <int LPT>
__global__ __launch_bounds__(256) void k_pg_zbuffer(PgFrame f) {
  const int lane = threadIdx.x & 63, sub = lane % LPT;
  const int32_t t = ((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6)) * (64 / LPT) + lane / LPT;
  bool live = t < f.T && f.tri_valid[t] != 0;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a;
  int x0 = 0, y0 = 0, bw = 0, bh = 0;
  if (live) {
    const int32_t ia = f.tris[3 * t], ib = f.tris[3 * t + 1], ic = f.tris[3 * t + 2];
    a = f.proj[ia]; b = f.proj[ib]; c = f.proj[ic];
    const float2 Pa = f.pos[ia], Pb = f.pos[ib], Pc = f.pos[ic];
    const float area_prev = pg_e(Pa.x, Pa.y, Pb.x, Pb.y, Pc.x, Pc.y);
    const float area_cur = pg_e(a.x, a.y, b.x, b.y, c.x, c.y);
    // (both non-zero and of one sign; a NaN area fails both comparisons)
    live = a.w != 0.f && b.w != 0.f && c.w != 0.f && ((area_prev > 0.f && area_cur > 0.f) || (area_prev < 0.f && area_cur < 0.f));
    int x1, y1;
    raster_span(fminf(a.x, fminf(b.x, c.x)), fmaxf(a.x, fmaxf(b.x, c.x)), f.W, x0, x1);
    raster_span(fminf(a.y, fminf(b.y, c.y)), fmaxf(a.y, fmaxf(b.y, c.y)), f.H, y0, y1);
    bw = x1 - x0 + 1; bh = y1 - y0 + 1;
    live = live && bw > 0 && bh > 0;
  }
  const int n = live ? bw * bh : 0;
  if (LPT == 64 || n <= 256) pg_cover(a, b, c, x0, y0, bw, n, sub, LPT, f.W, (uint32_t)t, f.key);
  if (LPT == 64) return;
  unsigned long long big = __ballot(n > 256 && sub == 0);
  while (big) {  // wave-uniform: every lane takes the triangle of lane l
    const int l = (int)__builtin_ctzll(big);
    big &= big - 1;
    const float4 la = make_float4(__shfl(a.x, l, 64), __shfl(a.y, l, 64), __shfl(a.z, l, 64), 1.f);
    const float4 lb = make_float4(__shfl(b.x, l, 64), __shfl(b.y, l, 64), __shfl(b.z, l, 64), 1.f);
    const float4 lc = make_float4(__shfl(c.x, l, 64), __shfl(c.y, l, 64), __shfl(c.z, l, 64), 1.f);
    pg_cover(la, lb, lc, __shfl(x0, l, 64), __shfl(y0, l, 64), __shfl(bw, l, 64), __shfl(n, l, 64), lane, 64, f.W,
             (uint32_t)__shfl(t, l, 64), f.key);
  }
}

__global__ __launch_bounds__(256) void k_pg_sample(PgFrame f) {
  const int q = (int)(blockIdx.x * 256 + threadIdx.x);
  if (q >= f.n) return;
  const float2 p = f.pix[q];
  const float fj = floorf(p.x + 0.5f), fi = floorf(p.y + 0.5f);
  float out = __builtin_nanf("");
  if (fj >= 0.f && fj < (float)f.W && fi >= 0.f && fi < (float)f.H) {  // (compared in float: a NaN or a huge pixel never reaches the conversion)
    const unsigned long long k = f.key[(size_t)(int)fi * f.W + (int)fj];
    if (k != 0ull) {
      const uint32_t t = 0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull);
      bool in;
      const float xi = pg_interp(f.proj[f.tris[3 * t]], f.proj[f.tris[3 * t + 1]], f.proj[f.tris[3 * t + 2]], p.x, p.y, in);
      if (pg_finite(xi) && xi > 0.f) out = xi;
    }
  }
  f.pred[q] = out;
}

__global__ __launch_bounds__(256) void k_pg_map(int64_t npix, const unsigned long long* __restrict__ key, float* __restrict__ map) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= npix) return;
  const unsigned long long v = key[k];
  map[k] = v != 0ull ? __uint_as_float((uint32_t)(v >> 32)) : __builtin_nanf("");
}

}  // namespace

void pg_launch_project(hipStream_t s, const PgFrame& f) {
  if (f.V > 0) hipLaunchKernelGGL(k_pg_project, dim3((f.V + 255) / 256), dim3(256), 0, s, f);
}

void pg_launch_zbuffer(hipStream_t s, const PgFrame& f) {
  if (f.T <= 0) return;
  if ((int64_t)f.W * f.H / f.T >= 64)  // mean triangle area in pixels (the dense raster's rule, kernels.hip launch_raster)
    hipLaunchKernelGGL(k_pg_zbuffer<64>, dim3((f.T + 3) / 4), dim3(256), 0, s, f);
  else
    hipLaunchKernelGGL(k_pg_zbuffer<8>, dim3((f.T + 31) / 32), dim3(256), 0, s, f);
}

void pg_launch_sample(hipStream_t s, const PgFrame& f) {
  if (f.n > 0) hipLaunchKernelGGL(k_pg_sample, dim3((f.n + 255) / 256), dim3(256), 0, s, f);
}

void pg_launch_map(hipStream_t s, int64_t npix, const unsigned long long* key, float* map) {
  if (npix > 0) hipLaunchKernelGGL(k_pg_map, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, npix, key, map);
}

}  // namespace flamehip
