// flame_ros_amd/csrc/frontend.hip -- kernels of the feature front end (gfx950): epipolar inverse-depth tracking, one wavefront
// per live feature with the lanes over the samples of its search (k_fe_track); gradient-maximum detection, one wavefront per
// grid cell (k_fe_detect); slot assignment of the detections and compaction of the emitted features (k_fe_compact); the hand-over
// of an evicted pose frame's features to the pose frame that takes its ring slot, one thread per slot (k_fe_carry).
//
// Arithmetic contract (DESIGN.md "Feature front end"): float32 with + - x / sqrtf floorf ceilf only, every operation rounded
// on its own (-ffp-contract=off, NO fmaf here: the restatement in tests/frontend_ref.py is NumPy, which has none), image costs
// are integers -- any reduction order gives the same bits.  The statement is this build's own ([UPSTREAM-RECALL] where it
// follows the paper); tests/frontend_ref.py restates it operation by operation and the GPU must equal it bit for bit.
//
// Memory: images are dense (row pitch = W) uint8, rows start at any byte address -- every pixel load is a byte load (a 640x480
// image stays in L2; no alignment is assumed).  No LDS in the tracker: a lane keeps the costs of its (up to 5) samples in
// registers, the winner's neighbours travel by lane shuffles.
#include "frontend.h"

namespace flamehip {

namespace {

constexpr unsigned long long kNone = ~0ull;

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
__device__ __forceinline__ bool fe_finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }

// Position of one sample in sixteenths of a pixel, the quantisation every sampler shares; false when it lies outside the image
// (the callers return at once then and never read the two integers: the test comes last so that they compile as they did inline).
__device__ __forceinline__ bool fe_sample_q(const FeFrame& f, float px, float py, int* qx, int* qy) {
  const float fqx = floorf(px * 16.0f + 0.5f), fqy = floorf(py * 16.0f + 0.5f);
  *qx = (int)fqx;
  *qy = (int)fqy;
  return fqx >= 0.0f && fqx <= (float)(16 * f.W) && fqy >= 0.0f && fqy <= (float)(16 * f.H);
}

// The three matching costs of a window, stated once for the upright and the warped sampler.  add(I, R) takes one window pixel:
// I = the bilinear sum of the current image, 256-scaled (0 ... 65 280), R = 256 ref (0 ... 65 280); cost() closes the sums.
// SSD: the sum of D_i^2 over the n = win^2 differences D_i = I_i - R_i (|D| <= 65 280: the square fits 32 bits).
// ZSSD (DESIGN.md 5.3 "Matching cost", mode ZSSD): with S1 = sum D_i (|S1| <= 81 * 65 280: an int32) and S2 = sum D_i^2, the cost
// is n S2 - S1^2 -- n^2 times the variance of D over the window, >= 0, <= (n^2 - 1) 65 280^2 < 2^45, and the same integer whatever
// constant a frame's exposure adds to every D_i.
// The gain-invariant cost (DESIGN.md 5.3 "Matching cost", flame_hip_frontend_set_gain_invariant): the residual of the reference
// window after the best fit ref ~ g cur + b.  SI = sum I (< 2^23), SII = sum I^2, SIR = sum I R (each term < 2^32, the sums < 2^39)
// and
//   ZI = n SII - SI^2 (>= 0, < 2^45),  ZIR = n SIR - SI SR (signed, |ZIR| < 2^45),  ZR = n SRR - SR^2 (>= 0, < 2^45)
// are exact integers; ZI == 0 (a flat current window) or ZIR <= 0 (anti-correlation is refused) leaves C = ZR, otherwise
//   C = floor(ZR - ZIR^2 / ZI), clamped at 0:
// a double multiply, divide and subtract on integers below 2^53, each rounded once (-ffp-contract=off) -- the bits of NumPy's
// float64.  C <= ZR < 2^45: the argmin key keeps its width.  The unit is ZSSD's (n^2 x a variance in 256-scaled grey levels).
template <int COST>
struct FeSums {
  unsigned long long S2 = 0, SIR = 0;  // sum D^2 (SSD, ZSSD) or sum I^2 (GI); sum I R (GI)
  int S1 = 0;                          // sum D (ZSSD) or sum I (GI)
  __device__ __forceinline__ void add(int I, int R) {
    if constexpr (COST == kFeCostGi) {
      S1 += I;
      S2 += (unsigned long long)((unsigned int)I * (unsigned int)I);  // (both products fit 32 bits)
      SIR += (unsigned long long)((unsigned int)I * (unsigned int)R);
    } else {
      const int D = I - R;
      const unsigned int aD = (unsigned int)(D < 0 ? -D : D);
      S2 += (unsigned long long)(aD * aD);
      if (COST == kFeCostZssd) S1 += D;
    }
  }
  // (SR, ZR): fe_ref_sums of the feature; the gain-invariant cost alone reads them
  __device__ __forceinline__ unsigned long long cost(int win, unsigned int SR, unsigned long long ZR) const {
    const unsigned long long n = (unsigned long long)(unsigned int)(win * win);
    if constexpr (COST == kFeCostGi) {
      const unsigned long long SI = (unsigned long long)(unsigned int)S1;
      const unsigned long long ZI = n * S2 - SI * SI;
      const long long ZIR = (long long)(n * SIR) - (long long)(SI * (unsigned long long)SR);
      if (ZI == 0ull || ZIR <= 0ll) return ZR;
      const double z = (double)ZIR;
      const double q = (z * z) / (double)ZI;
      const double Cd = (double)ZR - q;
      return Cd > 0.0 ? (unsigned long long)floor(Cd) : 0ull;
    } else if constexpr (COST == kFeCostZssd) {
      const unsigned int a1 = (unsigned int)(S1 < 0 ? -S1 : S1);
      return n * S2 - (unsigned long long)a1 * (unsigned long long)a1;
    } else {
      return S2;
    }
  }
};

// fe_ref_sums forms (SR, ZR) of the feature once, before the search: the 64 lanes cover the n <= 81 reference pixels in two
// passes, s1 = sum ref <= 81 * 255 and s2 = sum ref^2 <= 81 * 255^2 < 2^23 are int32 sums an xor butterfly leaves in every lane
// (any order: the same integers), SR = 256 s1 and ZR = 65536 (n s2 - s1^2).  The caller has tested that the window lies inside.
__device__ __forceinline__ void fe_ref_sums(const FeFrame& f, const uint8_t* __restrict__ ref, int u, int v, int lane, unsigned int* SR,
                                            unsigned long long* ZR) {
  const int r = f.win >> 1, n = f.win * f.win;
  int s1 = 0, s2 = 0;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int i = lane + 64 * pass;
    if (i < n) {
      const int q = ref[(size_t)(v - r + i / f.win) * f.W + (u - r + i % f.win)];
      s1 += q;
      s2 += q * q;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o, 64);
    s2 += __shfl_xor(s2, o, 64);
  }
  const unsigned int t1 = (unsigned int)__builtin_amdgcn_readfirstlane(s1), t2 = (unsigned int)__builtin_amdgcn_readfirstlane(s2);
  *SR = 256u * t1;  // (wave-uniform: both live in scalar registers through the search)
  *ZR = (unsigned long long)((unsigned int)n * t2 - t1 * t1) << 16;
}

// Cost of one sample on the upright window: the win x win bilinear window of the current image at p, quantised to 1/16 px, against
// the reference window under the cost COST; kNone when the window (with its +1 bilinear neighbours) leaves the image.  Per row
// two running pixels are carried, so a window pixel costs two loads of the current image and one of the reference patch.
template <int COST>
__device__ __forceinline__ unsigned long long fe_cost(const FeFrame& f, const uint8_t* __restrict__ ref, int u, int v, float px,
                                                      float py, unsigned int SR, unsigned long long ZR) {
  int qx, qy;
  if (!fe_sample_q(f, px, py, &qx, &qy)) return kNone;
  const int ix = qx >> 4, iy = qy >> 4;
  const int r = f.win >> 1;
  if (ix - r < 0 || iy - r < 0 || ix + r + 1 > f.W - 1 || iy + r + 1 > f.H - 1) return kNone;
  const int wx1 = qx & 15, wx0 = 16 - wx1, wy1 = qy & 15, wy0 = 16 - wy1;
  FeSums<COST> s;
  for (int dy = -r; dy <= r; ++dy) {
    const uint8_t* __restrict__ r0 = f.cur + (size_t)(iy + dy) * f.W + (ix - r);
    const uint8_t* __restrict__ r1 = r0 + f.W;
    const uint8_t* __restrict__ rr = ref + (size_t)(v + dy) * f.W + (u - r);
    int t0 = r0[0], b0 = r1[0];
    for (int dx = 0; dx < f.win; ++dx) {
      const int t1 = r0[dx + 1], b1 = r1[dx + 1];
      s.add(wy0 * (wx0 * t0 + wx1 * t1) + wy1 * (wx0 * b0 + wx1 * b1), 256 * (int)rr[dx]);
      t0 = t1;
      b0 = b1;
    }
  }
  return s.cost(f.win, SR, ZR);
}

// The warped window (DESIGN.md 5.3 "Warped window", flame_hip_frontend_set_warp): the current image is sampled where the reference
// window's pixels land under the pose change, an affine map J taken once per feature at the prior clamped into the searched
// interval.  fe_warp_jq forms J = d(projection)/d(reference pixel) in float32 (no fmaf; gx_r = A[r][0] / fx, gy_r = A[r][1] / fy
// are the derivatives of a = A b), quantises each entry to 1/256 (Jq = floorf(256 J + 0.5f), refused unless that float is finite
// and at most 1024 in magnitude: a stretch of 4) and tests det Jq >= 4096 (an area scale of 1/16; no mirrored or collapsed map).
// Everything here is wave-uniform: the caller keeps the four integers and the verdict in scalar registers.
struct FeJq {
  int j00, j01, j10, j11;
};
__device__ __forceinline__ bool fe_warp_q(float J, int* q) {
  const float fq = floorf(J * 256.0f + 0.5f);
  const bool ok = __builtin_fabsf(fq) <= 1024.0f;  // (a NaN fails, an infinity fails)
  *q = __builtin_amdgcn_readfirstlane(ok ? (int)fq : 0);
  return ok;
}
__device__ __forceinline__ bool fe_warp_jq(const FeFrame& f, const FePose& P, float a0, float a1, float a2, float mu, float xi0,
                                           float xi1, FeJq* Jq) {
  const float t = mu > xi0 ? mu : xi0;
  const float xj = t < xi1 ? t : xi1;
  const float w0 = a0 + xj * P.c[0], w1 = a1 + xj * P.c[1], w2 = a2 + xj * P.c[2];
  const float px = w0 / w2, py = w1 / w2;
  const float gx0 = P.A[0] / f.fx, gx1 = P.A[3] / f.fx, gx2 = P.A[6] / f.fx;
  const float gy0 = P.A[1] / f.fy, gy1 = P.A[4] / f.fy, gy2 = P.A[7] / f.fy;
  bool ok = fe_warp_q((gx0 - px * gx2) / w2, &Jq->j00);
  ok = fe_warp_q((gy0 - px * gy2) / w2, &Jq->j01) && ok;
  ok = fe_warp_q((gx1 - py * gx2) / w2, &Jq->j10) && ok;
  ok = fe_warp_q((gy1 - py * gy2) / w2, &Jq->j11) && ok;
  const int det = Jq->j00 * Jq->j11 - Jq->j01 * Jq->j10;  // (|.| <= 2^21)
  return __builtin_amdgcn_readfirstlane((int)(ok && det >= 4096)) != 0;
}

// Cost of one sample under the warp, the one sampler of the three costs: window offset (i, j) of the reference window is compared
// with the current image at (qx, qy) + ((Jq (i, j) + 8) >> 4) sixteenths of a pixel (an arithmetic shift: it floors), bilinear
// with that position's own sixteenths -- four byte loads per window pixel.  The offsets are floors of a map linear in i and in j,
// so their extremes over the window sit at its four corners: testing the corners (and their +1 neighbours) tests every pixel.
// Jq = (256, 0, 0, 256) gives ox = qx + 16 i: the unwarped integers.  I feeds FeSums<COST> exactly as in fe_cost: its bounds
// hold unchanged (I <= 65 280).
template <int COST>
__device__ __forceinline__ unsigned long long fe_cost_warp(const FeFrame& f, const uint8_t* __restrict__ ref, int u, int v, float px,
                                                           float py, const FeJq& Jq, unsigned int SR, unsigned long long ZR) {
  int qx, qy;
  if (!fe_sample_q(f, px, py, &qx, &qy)) return kNone;
  const int r = f.win >> 1;
#pragma unroll
  for (int corner = 0; corner < 4; ++corner) {
    const int i = corner & 1 ? r : -r, j = corner & 2 ? r : -r;
    const int x = (qx + ((Jq.j00 * i + Jq.j01 * j + 8) >> 4)) >> 4, y = (qy + ((Jq.j10 * i + Jq.j11 * j + 8) >> 4)) >> 4;
    if (x < 0 || y < 0 || x + 1 > f.W - 1 || y + 1 > f.H - 1) return kNone;
  }
  FeSums<COST> s;
  for (int j = -r; j <= r; ++j) {
    const uint8_t* __restrict__ rr = ref + (size_t)(v + j) * f.W + u;
    for (int i = -r; i <= r; ++i) {
      const int ox = qx + ((Jq.j00 * i + Jq.j01 * j + 8) >> 4), oy = qy + ((Jq.j10 * i + Jq.j11 * j + 8) >> 4);
      const uint8_t* __restrict__ q = f.cur + (size_t)(oy >> 4) * f.W + (ox >> 4);
      const int wx1 = ox & 15, wx0 = 16 - wx1, wy1 = oy & 15, wy0 = 16 - wy1;
      const int I = wy0 * (wx0 * (int)q[0] + wx1 * (int)q[1]) + wy1 * (wx0 * (int)q[f.W] + wx1 * (int)q[f.W + 1]);  // <= 65 280
      s.add(I, 256 * (int)rr[i]);
    }
  }
  return s.cost(f.win, SR, ZR);
}

// The reference-patch gradient gate (DESIGN.md 5.3 "Reference-patch gradient"): does the win x win reference window have structure
// ALONG the epipolar line?  The 64 lanes cover the n <= 81 window pixels in two passes; the three sums of the structure tensor are
// integers (each <= 81 * 255^2 < 2^24: exact as float32) and an xor butterfly leaves them in every lane, so the result is
// wave-uniform.  (dx, dy) is the direction from the feature's pixel to the current view's epipole, homogeneous: no division, the
// sign does not matter.  Passes iff Q >= thr N, i.e. the mean square of the directional derivative is at least min_grad^2 (a
// central difference is twice the gradient); a NaN refuses.  kFeOutside when the one-pixel ring around the window leaves the image.
__device__ __forceinline__ int fe_ref_grad(const FeFrame& f, const uint8_t* __restrict__ ref, int p, int u, int v, int lane) {
  const int r = f.win >> 1, n = f.win * f.win;
  if (u - r - 1 < 0 || v - r - 1 < 0 || u + r + 1 > f.W - 1 || v + r + 1 > f.H - 1) return kFeOutside;
  int sxx = 0, sxy = 0, syy = 0;
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    const int i = lane + 64 * pass;
    if (i < n) {
      const uint8_t* __restrict__ q = ref + (size_t)(v - r + i / f.win) * f.W + (u - r + i % f.win);
      const int gx = (int)q[1] - (int)q[-1], gy = (int)q[f.W] - (int)q[-f.W];
      sxx += gx * gx;
      sxy += gx * gy;
      syy += gy * gy;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sxx += __shfl_xor(sxx, o, 64);
    sxy += __shfl_xor(sxy, o, 64);
    syy += __shfl_xor(syy, o, 64);
  }
  const FeEpi e = f.epi[p];
  const float dx = e.E[0] - (float)u * e.E[2], dy = e.E[1] - (float)v * e.E[2];
  const float Q = ((dx * dx) * (float)sxx + (2.0f * (dx * dy)) * (float)sxy) + (dy * dy) * (float)syy;
  const float N = dx * dx + dy * dy;
  const float thr = (4.0f * (float)n) * (f.min_epi_grad * f.min_epi_grad);
  return Q >= thr * N ? kFeOk : kFeRefGrad;
}

__global__ __launch_bounds__(256) void k_fe_kill(FeFrame f, unsigned long long valid_mask) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= f.max_features) return;
  if (f.alive[slot] && !((valid_mask >> f.pf[slot]) & 1ull)) f.alive[slot] = 0;
}

// COST picks the matching cost (kFeCostSsd, kFeCostZssd, kFeCostGi: the gain-invariant one); f.bad_match_cost is the host's
// threshold for that cost.  Everything behind the cost -- argmin, BAD_MATCH, AMBIGUOUS, the parabola -- takes it as it comes; the
// gain-invariant cost adds one decision, BAD_MATCH for a flat reference window (ZR == 0: nothing to correlate).  RG puts the
// reference-patch gradient gate between the NO_PARALLAX test and the search; the instantiations without it hold none of its code.
// WARP samples the current image through the feature's quantised affine map (fe_warp_jq, fe_cost_warp) and refuses, behind the
// gradient gate and before the search, a feature whose map is out of range: OUTSIDE, counted in counts[13] as well, no search
// record.  The instantiations without it hold none of its code either.
template <int COST, bool RG, bool WARP>
__global__ __launch_bounds__(256) void k_fe_track(FeFrame f) {
  const int lane = threadIdx.x & 63;
  const int slot = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (slot >= f.max_features) return;  // (whole wavefronts leave: everything below is wave-level)
  if (!f.alive[slot]) {
    if (lane == 0) {
      f.status[slot] = kFeFree;
      f.kstar[slot] = -1;
      f.cell_of[slot] = -1;
      f.seg[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      f.steps[slot] = 0;
    }
    return;
  }
  const int u = f.u[slot], v = f.v[slot], p = f.pf[slot];
  float mu = f.mu[slot], var = f.var[slot];
  int drop = f.drop[slot];
  const FePose P = f.poses[p];
  const uint8_t* __restrict__ ref = f.imgs + (size_t)p * f.W * f.H;

  const float b0 = ((float)u - f.cx) / f.fx, b1 = ((float)v - f.cy) / f.fy;
  const float a0 = (P.A[0] * b0 + P.A[1] * b1) + P.A[2];
  const float a1 = (P.A[3] * b0 + P.A[4] * b1) + P.A[5];
  const float a2 = (P.A[6] * b0 + P.A[7] * b1) + P.A[8];
  const float c0 = P.c[0], c1 = P.c[1], c2 = P.c[2];
  const float two = 2.0f * sqrtf(var);
  const float lo = mu - two, hi = mu + two;
  const float xi0 = lo > f.idepth_min ? lo : f.idepth_min;
  const float xi1 = hi < f.idepth_max ? hi : f.idepth_max;
  const float d0 = a2 + xi0 * c2, d1 = a2 + xi1 * c2;
  const int r = f.win >> 1;
  const bool ref_in = u - r >= 0 && v - r >= 0 && u + r <= f.W - 1 && v + r <= f.H - 1;

  int status, ks = -1;
  float mu_new = mu, var_new = var;
  float4 seg = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // the search record: stays zero when no search runs
  int steps = 0;
  bool warp_refused = false;
  if (!(d0 > 0.0f && d1 > 0.0f) || !ref_in) {
    status = kFeOutside;  // an end of the search lies behind the camera / the reference patch leaves its image
  } else {
    const float x0 = (a0 + xi0 * c0) / d0, y0 = (a1 + xi0 * c1) / d0;
    const float x1 = (a0 + xi1 * c0) / d1, y1 = (a1 + xi1 * c1) / d1;
    const float dx = x1 - x0, dy = y1 - y0;
    const float L = sqrtf(dx * dx + dy * dy);
    int rg = kFeOk;
    FeJq Jq = {256, 0, 0, 256};
    if (!(L >= 2.0f)) {
      status = kFeNoParallax;
    } else if (RG && (rg = fe_ref_grad(f, ref, p, u, v, lane)) != kFeOk) {
      status = rg;  // no structure along the epipolar line (or the window's ring leaves the image): no search, a failure
    } else if (WARP && !fe_warp_jq(f, P, a0, a1, a2, mu, xi0, xi1, &Jq)) {
      status = kFeOutside;  // the window's map is out of range (stretch > 4, area < 1/16, mirrored): no search, a failure
      warp_refused = true;
    } else {
      const int S = L >= (float)kFeMaxSamples ? kFeMaxSamples : (int)ceilf(L);
      const float ex = dx / (float)S, ey = dy / (float)S;
      seg = make_float4(x0, y0, ex, ey);
      steps = S;
      unsigned long long C[kFePasses];
      unsigned long long best = kNone;
      unsigned int SR = 0u;
      unsigned long long ZR = 0ull;
      if (COST == kFeCostGi) fe_ref_sums(f, ref, u, v, lane, &SR, &ZR);
#pragma unroll
      for (int pass = 0; pass < kFePasses; ++pass) {
        const int k = lane + 64 * pass;
        unsigned long long c = kNone;
        if (64 * pass <= S && k <= S) {
          if constexpr (WARP) c = fe_cost_warp<COST>(f, ref, u, v, x0 + (float)k * ex, y0 + (float)k * ey, Jq, SR, ZR);
          else c = fe_cost<COST>(f, ref, u, v, x0 + (float)k * ex, y0 + (float)k * ey, SR, ZR);
        }
        C[pass] = c;
        if (c != kNone) {  // (c < 2^39 -- ZSSD, GI: c < 2^45 --, k < 2^9: one 64-bit key < 2^54 orders by cost, then by k)
          const unsigned long long key = (c << 9) | (unsigned long long)k;
          best = key < best ? key : best;
        }
      }
      best = wave_min_u64(best);
      if (best == kNone) {
        status = kFeOutside;
      } else {
        ks = (int)(best & 511ull);
        const unsigned long long Cbest = best >> 9;
        if ((COST == kFeCostGi && ZR == 0ull) || Cbest > f.bad_match_cost) {
          status = kFeBadMatch;
        } else {
          bool amb = false;
#pragma unroll
          for (int pass = 0; pass < kFePasses; ++pass) {
            const int k = lane + 64 * pass;
            const int dk = k > ks ? k - ks : ks - k;
            if (C[pass] != kNone && dk > 2 && 2ull * C[pass] < 3ull * Cbest) amb = true;
          }
          if (__ballot(amb) != 0ull) {
            status = kFeAmbiguous;
          } else {
            // the winner's neighbours: sample k sits in lane k & 63, pass k >> 6 (k > S holds kNone already)
            unsigned long long Cm = kNone, Cp = kNone;
            {
              const int km = ks > 0 ? ks - 1 : 0, kp = ks + 1;
              unsigned long long sm = C[0], sp = C[0];
#pragma unroll
              for (int pass = 1; pass < kFePasses; ++pass) {
                if ((km >> 6) == pass) sm = C[pass];
                if ((kp >> 6) == pass) sp = C[pass];
              }
              sm = __shfl(sm, km & 63, 64);
              sp = __shfl(sp, kp & 63, 64);
              if (ks > 0) Cm = sm;
              Cp = sp;
            }
            float delta = 0.0f;
            if (Cm != kNone && Cp != kNone) {
              const float fm = (float)Cm, f0 = (float)Cbest, fp = (float)Cp;
              const float den = (fm - 2.0f * f0) + fp;
              if (den > 0.0f) delta = (0.5f * (fm - fp)) / den;
            }
            const float t = (float)ks + delta;
            const float xs = x0 + t * ex, ys = y0 + t * ey;
            const bool xdom = __builtin_fabsf(ex) >= __builtin_fabsf(ey);
            float xi_m, xi_p, xi_n;
            if (xdom) {
              const float xp = xs + ex, xn = xs - ex;
              xi_m = (a0 - xs * a2) / (xs * c2 - c0);
              xi_p = (a0 - xp * a2) / (xp * c2 - c0);
              xi_n = (a0 - xn * a2) / (xn * c2 - c0);
            } else {
              const float yp = ys + ey, yn = ys - ey;
              xi_m = (a1 - ys * a2) / (ys * c2 - c1);
              xi_p = (a1 - yp * a2) / (yp * c2 - c1);
              xi_n = (a1 - yn * a2) / (yn * c2 - c1);
            }
            const float s = (xi_p - xi_n) * 0.5f;
            const float var_m = (s * s) * f.epipolar_line_var;
            const float den = var + var_m;
            const float mu_f = (mu * var_m + xi_m * var) / den;
            const float var_f = (var * var_m) / den;
            if (fe_finite(xi_m) && fe_finite(var_m) && fe_finite(mu_f) && fe_finite(var_f)) {
              status = kFeOk;
              mu_new = mu_f;
              var_new = var_f;
            } else {
              status = kFeBadMatch;  // a degenerate measurement (the search ran along a line of constant inverse depth)
            }
          }
        }
      }
    }
  }

  const bool failed = status == kFeOutside || status == kFeBadMatch || status == kFeAmbiguous || (RG && status == kFeRefGrad);
  if (status == kFeOk) {
    mu = mu_new;
    var = var_new;
    drop = 0;
  }
  // projection into the current frame
  const float w0 = a0 + mu * c0, w1 = a1 + mu * c1, w2 = a2 + mu * c2;
  bool pok = false;
  float px = 0.0f, py = 0.0f, xc = 0.0f, vc = 0.0f;
  if (w2 > 0.0f) {
    px = w0 / w2;
    py = w1 / w2;
    xc = mu / w2;
    const float g = a2 / (w2 * w2);
    vc = var * (g * g);
    pok = px >= 0.0f && px <= (float)(f.W - 1) && py >= 0.0f && py <= (float)(f.H - 1) && fe_finite(xc) && fe_finite(vc) &&
          vc >= 0.0f;
  }
  // the letterbox: a projection outside the band of rows fails like one outside the image (the band is the image without one)
  const bool refused = pok && !(py >= (float)f.gates.y_lo && py <= (float)(f.gates.y_hi - 1));
  pok = pok && !refused;
  if (failed || !pok) drop += 1;
  const bool dies = drop > f.max_dropouts;
  if (lane == 0) {
    f.mu[slot] = mu;
    f.var[slot] = var;
    f.drop[slot] = drop;
    f.kstar[slot] = ks;
    f.seg[slot] = seg;
    f.steps[slot] = steps;
    atomicAdd(&f.counts[RG && status == kFeRefGrad ? 12 : 2 + status], 1);
    if (refused) atomicAdd(&f.counts[11], 1);
    if (WARP && warp_refused) atomicAdd(&f.counts[13], 1);
    if (dies) {
      f.alive[slot] = 0;
      f.status[slot] = kFeDied;
      f.cell_of[slot] = -1;
      atomicAdd(&f.counts[2 + kFeDied], 1);
    } else {
      f.status[slot] = status;
      int cell = -1;
      if (pok) {
        cell = ((int)py / f.dws) * f.ncx + (int)px / f.dws;
        bool held = false;
        if (f.gates.height_gate) {  // height of the feature's world point along the caller's up vector (a NaN height is held)
          const float bx = (px - f.cx) / f.fx, by = (py - f.cy) / f.fy;
          const float height = ((f.gates.hr0 * bx + f.gates.hr1 * by) + f.gates.hr2) / xc + f.gates.h0;
          held = !(height >= f.gates.min_height && height <= f.gates.max_height);
        }
        if (held) {
          // not emitted and no candidate of its cell, but the cell stays occupied for the detection (every holder stores 0)
          f.cell_held[cell] = 0;
          atomicAdd(&f.counts[10], 1);
          cell = -1;
        } else {
          // one emitted feature per cell: smallest variance, then lowest slot
          atomicMin(&f.cell_key[cell], ((unsigned long long)__float_as_uint(vc) << 32) | (unsigned long long)(unsigned int)slot);
          f.proj[slot] = make_float4(px, py, xc, vc);
        }
      }
      f.cell_of[slot] = cell;
    }
  }
}

// One wavefront per cell: the cell's largest squared central-difference gradient, ties to the smallest y, then the smallest x.
__global__ __launch_bounds__(256) void k_fe_detect(FeFrame f) {
  const int lane = threadIdx.x & 63;
  const int cell = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cell >= f.ncx * f.ncy) return;
  // occupied by an emitted feature of this frame, or by one the height gate holds
  if (f.cell_key[cell] != kNone || (f.gates.height_gate && f.cell_held[cell] == 0)) {
    if (lane == 0) f.det[cell] = -1;
    return;
  }
  const int ccx = cell % f.ncx, ccy = cell / f.ncx, m = (f.win >> 1) + 1;
  const int xlo = max(ccx * f.dws, m), xhi = min(ccx * f.dws + f.dws, f.W - m);
  const int ylo = max(max(ccy * f.dws, m), f.gates.y_lo), yhi = min(min(ccy * f.dws + f.dws, f.H - m), f.gates.y_hi);
  const int cw = xhi - xlo, ch = yhi - ylo;
  unsigned long long best = 0ull;
  if (cw > 0 && ch > 0) {
    for (int i = lane; i < cw * ch; i += 64) {
      const int y = ylo + i / cw, x = xlo + i % cw;
      const uint8_t* __restrict__ q = f.cur + (size_t)y * f.W + x;
      const int gx = (int)q[1] - (int)q[-1], gy = (int)q[f.W] - (int)q[-f.W];
      const unsigned long long key = ((unsigned long long)(unsigned int)(gx * gx + gy * gy) << 32) |
                                     ((unsigned long long)(0xFFFF - y) << 16) | (unsigned long long)(0xFFFF - x);
      best = key > best ? key : best;
    }
  }
  best = wave_max_u64(best);
  if (lane == 0) {
    const int g2 = (int)(best >> 32);
    f.det[cell] = g2 >= f.g2_min ? ((0xFFFF - (int)((best >> 16) & 0xFFFFull)) << 16) | (0xFFFF - (int)(best & 0xFFFFull)) : -1;
  }
}

// exclusive rank of the set flags over the block's 1024 threads, and their number
__device__ __forceinline__ int fe_block_rank(bool flag, int* s_w, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  const int within = __popcll(b & ((1ull << lane) - 1ull));
  __syncthreads();  // (the previous call's readers are done)
  if (lane == 0) s_w[wv] = __popcll(b);
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = s_w[i];
    if (i < wv) base += c;
    tot += c;
  }
  *total = tot;
  return base + within;
}

// ONE workgroup: on a pose frame the detections take the free slots (ascending slots, cells in row-major order); then the emitted
// features -- the winner of every cell -- are compacted in ascending slot order.
__global__ __launch_bounds__(1024) void k_fe_compact(FeFrame f) {
  __shared__ int s_w[16];
  const int tid = threadIdx.x;
  int n_new = 0, n_dropped = 0;
  if (f.is_poseframe) {
    int nfree = 0, ndet = 0, tot = 0;
    for (int base = 0; base < f.max_features; base += 1024) {
      const int slot = base + tid;
      const bool fr = slot < f.max_features && !f.alive[slot];
      const int rk = fe_block_rank(fr, s_w, &tot);
      if (fr) f.freelist[nfree + rk] = slot;
      nfree += tot;
    }
    __syncthreads();
    const int ncells = f.ncx * f.ncy;
    for (int base = 0; base < ncells; base += 1024) {
      const int cell = base + tid;
      const int d = cell < ncells ? f.det[cell] : -1;
      const int rk = fe_block_rank(d >= 0, s_w, &tot);
      if (d >= 0 && ndet + rk < nfree) {
        const int slot = f.freelist[ndet + rk];
        const int x = d & 0xFFFF, y = d >> 16;
        f.alive[slot] = 1;
        f.u[slot] = x;
        f.v[slot] = y;
        f.pf[slot] = f.cur_pf;
        f.drop[slot] = 0;
        f.mu[slot] = f.idepth_init;
        f.var[slot] = f.var_init;
        f.status[slot] = kFeNew;
        f.kstar[slot] = -1;
        f.seg[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // (the slot may have died in this very frame: its search goes with it)
        f.steps[slot] = 0;
        f.cell_of[slot] = cell;
        f.proj[slot] = make_float4((float)x, (float)y, f.idepth_init, f.var_init);
        f.cell_key[cell] = ((unsigned long long)__float_as_uint(f.var_init) << 32) | (unsigned long long)(unsigned int)slot;
      }
      ndet += tot;
    }
    __syncthreads();
    n_new = ndet < nfree ? ndet : nfree;
    n_dropped = ndet - n_new;
  }
  int nout = 0, nlive = 0, tot = 0;
  for (int base = 0; base < f.max_features; base += 1024) {
    const int slot = base + tid;
    const bool al = slot < f.max_features && f.alive[slot];
    const int c = al ? f.cell_of[slot] : -1;
    const bool emit = c >= 0 && (unsigned int)(f.cell_key[c] & 0xFFFFFFFFull) == (unsigned int)slot;
    const int rk = fe_block_rank(emit, s_w, &tot);
    if (emit) {
      const float4 pr = f.proj[slot];
      FeOut o;
      o.x = pr.x; o.y = pr.y; o.mu = pr.z; o.var = pr.w;
      o.slot = slot;
      o.status = f.status[slot];
      f.out[nout + rk] = o;
    }
    nout += tot;
    (void)fe_block_rank(al, s_w, &tot);
    nlive += tot;
  }
  if (tid == 0) {
    f.counts[0] = nout;
    f.counts[1] = nlive;
    f.counts[2 + kFeNew] = n_new;
    f.counts[9] = n_dropped;
  }
}

// The hand-over (DESIGN.md 5.3 "Hand-over", flame_hip_frontend_set_carry): behind k_fe_compact of a pose frame that takes the ring
// slot f.cur_pf while the slot is in use.  One thread per slot; the old pose frame's features are the live slots of that ring slot
// that are not NEW.  One of them that this frame emitted (status OK or NO_PARALLAX, winner of its cell) at a pixel where k_fe_detect
// could have put a detection is carried: the emitted projection, rounded to the pixel, becomes its reference pixel and its prior --
// copies of the frame's own bits, two floorf, integer compares.  Every other one dies here (alive alone is written).
__global__ __launch_bounds__(256) void k_fe_carry(FeFrame f) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= f.max_features) return;
  if (!f.alive[slot] || f.pf[slot] != f.cur_pf) return;
  const int status = f.status[slot];
  if (status == kFeNew) return;
  bool carried = false;
  const int cell = f.cell_of[slot];
  if ((status == kFeOk || status == kFeNoParallax) && cell >= 0 &&
      (unsigned int)(f.cell_key[cell] & 0xFFFFFFFFull) == (unsigned int)slot) {
    const float4 pr = f.proj[slot];
    const int ur = (int)floorf(pr.x + 0.5f), vr = (int)floorf(pr.y + 0.5f), m = (f.win >> 1) + 1;
    if (ur >= m && ur < f.W - m && vr >= max(m, f.gates.y_lo) && vr < min(f.H - m, f.gates.y_hi)) {
      f.u[slot] = ur;
      f.v[slot] = vr;
      f.mu[slot] = pr.z;
      f.var[slot] = pr.w;
      carried = true;
    }
  }
  if (!carried) f.alive[slot] = 0;
  atomicAdd(&f.counts[carried ? 14 : 15], 1);
}

}  // namespace

void fe_launch_carry(hipStream_t s, const FeFrame& f) {
  hipLaunchKernelGGL(k_fe_carry, dim3((f.max_features + 255) / 256), dim3(256), 0, s, f);
}
void fe_launch_kill(hipStream_t s, const FeFrame& f, unsigned long long valid_mask) {
  hipLaunchKernelGGL(k_fe_kill, dim3((f.max_features + 255) / 256), dim3(256), 0, s, f, valid_mask);
}
template <bool RG, bool WARP>
static void fe_launch_track_cost(hipStream_t s, const FeFrame& f, int cost) {
  const dim3 grid((f.max_features + 3) / 4), block(256);
  if (cost == kFeCostGi) hipLaunchKernelGGL((k_fe_track<kFeCostGi, RG, WARP>), grid, block, 0, s, f);
  else if (cost == kFeCostZssd) hipLaunchKernelGGL((k_fe_track<kFeCostZssd, RG, WARP>), grid, block, 0, s, f);
  else hipLaunchKernelGGL((k_fe_track<kFeCostSsd, RG, WARP>), grid, block, 0, s, f);
}
void fe_launch_track(hipStream_t s, const FeFrame& f, int cost, bool ref_grad, bool warp) {
  if (warp) {
    if (ref_grad) fe_launch_track_cost<true, true>(s, f, cost);
    else fe_launch_track_cost<false, true>(s, f, cost);
  } else {
    if (ref_grad) fe_launch_track_cost<true, false>(s, f, cost);
    else fe_launch_track_cost<false, false>(s, f, cost);
  }
}
void fe_launch_detect(hipStream_t s, const FeFrame& f) {
  hipLaunchKernelGGL(k_fe_detect, dim3((f.ncx * f.ncy + 3) / 4), dim3(256), 0, s, f);
}
void fe_launch_compact(hipStream_t s, const FeFrame& f) {
  hipLaunchKernelGGL(k_fe_compact, dim3(1), dim3(1024), 0, s, f);
}

}  // namespace flamehip
