// flame_ros_amd/csrc/frontend.h -- the feature front end on the GPU: gradient-maximum detection on a cell grid and epipolar
// inverse-depth tracking (the first two stages of upstream's Flame::update()).  Kernels: frontend.hip; C ABI:
// frontend.cpp (include/flame_hip.h, flame_hip_frontend_*); the algorithm statement: DESIGN.md "Feature front end".
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flamehip {

constexpr int kFeMaxSamples = 256;    // S <= 256 steps, i.e. up to 257 samples of a search = 5 passes of the 64 lanes
constexpr int kFePasses = 5;
constexpr int kFeMaxPoseframes = 64;  // the ring's valid slots travel as one 64-bit mask
constexpr int kFeMaxWin = 9;

// per-slot status of the last frame (FLAME_HIP_FE_* of include/flame_hip.h)
enum { kFeOk = 0, kFeNoParallax = 1, kFeOutside = 2, kFeBadMatch = 3, kFeAmbiguous = 4, kFeNew = 5, kFeDied = 6, kFeRefGrad = 7, kFeFree = -1 };
constexpr int kFeCounts = 16;  // counts[]: 0 = emitted, 1 = live, 2 + status = features of that status (0..6), 9 = detections dropped (no free slot),
                               // 10 = features held by the height gate, 11 = projections refused by the letterbox,
                               // 12 = features of status kFeRefGrad (2 + 7 is taken),
                               // 13 = features the warped window refused (they are among the kFeOutside ones as well),
                               // 14 / 15 = features of the evicted pose frame the hand-over carried / lost (k_fe_carry)

// A = K R and c = K t of T_cur_ref, rounded once to float32 on the host (one record per pose-frame ring slot)
struct FePose {
  float A[9];
  float c[3];
};

// A = K R, c = K t of T_cur_ref = T_world_cur^-1 T_world_ref (row-major [R|t]), in double, each entry rounded once to float32.
// (Sums run left to right; tests/frontend_ref.py pose_record() is the same statement.)  The front end's pose table and the
// prediction stage (predict.h) both take their warp from here.
inline void pose_record(double fx, double fy, double cx, double cy, const double* Tc, const double* Tr, FePose* out) {
  double R[9], t[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (Tc[0 * 4 + i] * Tr[0 * 4 + j] + Tc[1 * 4 + i] * Tr[1 * 4 + j]) + Tc[2 * 4 + i] * Tr[2 * 4 + j];
    const double d0 = Tr[3] - Tc[3], d1 = Tr[7] - Tc[7], d2 = Tr[11] - Tc[11];
    t[i] = (Tc[0 * 4 + i] * d0 + Tc[1 * 4 + i] * d1) + Tc[2 * 4 + i] * d2;
  }
  for (int j = 0; j < 3; ++j) {
    out->A[0 + j] = (float)(fx * R[0 + j] + cx * R[6 + j]);
    out->A[3 + j] = (float)(fy * R[3 + j] + cy * R[6 + j]);
    out->A[6 + j] = (float)R[6 + j];
  }
  out->c[0] = (float)(fx * t[0] + cx * t[2]);
  out->c[1] = (float)(fy * t[1] + cy * t[2]);
  out->c[2] = (float)t[2];
}

// The epipole of the current view in a pose frame's image, homogeneous (DESIGN.md 5.3 "Reference-patch gradient"): with o = R_ref^T
// (t_cur - t_ref) the current camera's centre in the reference frame, E = (fx o0 + cx o2, fy o1 + cy o2, o2).  One record per
// pose-frame ring slot in a table of its own behind the pose table (FePose keeps its layout: predict.h shares it); formed and
// uploaded only while the gate is on.
struct FeEpi {
  float E[3];
};

// E of T_world_cur = Tc seen from T_world_ref = Tr (row-major [R|t]), in double, sums left to right, each entry rounded once to
// float32 (tests/fe_rg_ref.py epipole_record() is the same statement).
inline void epipole_record(double fx, double fy, double cx, double cy, const double* Tc, const double* Tr, FeEpi* out) {
  const double d0 = Tc[3] - Tr[3], d1 = Tc[7] - Tr[7], d2 = Tc[11] - Tr[11];
  double o[3];
  for (int i = 0; i < 3; ++i) o[i] = (Tr[0 * 4 + i] * d0 + Tr[1 * 4 + i] * d1) + Tr[2 * 4 + i] * d2;
  out->E[0] = (float)(fx * o[0] + cx * o[2]);
  out->E[1] = (float)(fy * o[1] + cy * o[2]);
  out->E[2] = (float)o[2];
}

// one emitted feature (the frame's output record, compacted in ascending slot order)
struct FeOut {
  float x, y, mu, var;
  int32_t slot, status;
};

// The gates of a frame (DESIGN.md 5.3 "Gates"), by value in FeFrame.  The letterbox band is the rows y_lo <= y < y_hi; without a
// letterbox it is the whole image (y_lo = 0, y_hi = H), which leaves every test what it was.  The height of a projected feature is
// ((hr0 bx + hr1 by) + hr2) / idepth + h0 with b = K^-1 (px, py, 1): hr = n^T R and h0 = n . t of T_world_cam, formed in double on
// the host and rounded once to float32.
struct FeGates {
  int32_t y_lo, y_hi, height_gate;
  float min_height, max_height, hr0, hr1, hr2, h0;
};

struct FeFrame {
  // geometry and parameters of this call
  int32_t W, H, max_features, win, dws, ncx, ncy, max_dropouts, g2_min, is_poseframe, cur_pf;
  float fx, fy, cx, cy, idepth_min, idepth_max, idepth_init, var_init, epipolar_line_var;
  uint64_t bad_match_cost;
  // images: ring slot p at imgs + p * W * H (dense rows); the current image is one of them or the extra slot
  const uint8_t* imgs;
  const uint8_t* cur;
  const FePose* poses;
  // feature state, one entry per slot
  uint8_t* alive;
  int32_t* u;
  int32_t* v;
  int32_t* pf;
  int32_t* drop;
  float* mu;
  float* var;
  // per-frame results per slot
  int32_t* status;
  int32_t* kstar;
  int32_t* cell_of;  // detection cell of the projected feature, -1 = not a candidate for emission
  float4* proj;      // {x, y, idepth, var} in the current frame
  // per-frame grids and lists
  unsigned long long* cell_key;  // per cell: min over candidates of (bits(var_cur) << 32 | slot); all ones = empty
  int32_t* cell_held;            // per cell, behind cell_key and cleared with it: all ones = no holder, 0 = a feature the height gate holds projects here
  int32_t* det;                  // per cell: y << 16 | x of the detection, -1 = none
  int32_t* freelist;             // max_features
  FeOut* out;                    // max_features
  int32_t* counts;               // kFeCounts
  // the search record of the frame (debug images, flame_hip_frontend_searches): zero for a slot that ran no search
  float4* seg;     // {x0, y0, ex, ey}: sample k of the search sits at (x0 + k ex, y0 + k ey)
  int32_t* steps;  // S (0 = no search ran: free, NO_PARALLAX, OUTSIDE before the segment exists, NEW)
  FeGates gates;
  // the reference-patch gradient gate (read by the RG instantiations of k_fe_track only): min_grad, and the epipole table
  float min_epi_grad;
  const FeEpi* epi;
};

void fe_launch_kill(hipStream_t s, const FeFrame& f, unsigned long long valid_mask);
// cost: the matching cost of the frame (f.bad_match_cost is that cost's threshold); ref_grad: the reference-patch gradient gate (f.min_epi_grad, f.epi)
// warp: the warped window (reads nothing beyond poses, fx, fy; counts[13])
enum { kFeCostSsd = 0, kFeCostZssd = 1, kFeCostGi = 2 };
void fe_launch_track(hipStream_t s, const FeFrame& f, int cost, bool ref_grad, bool warp);
void fe_launch_detect(hipStream_t s, const FeFrame& f);
void fe_launch_compact(hipStream_t s, const FeFrame& f);
// the hand-over behind k_fe_compact of an evicting pose frame (DESIGN.md 5.3 "Hand-over"): the evicted ring slot is f.cur_pf; counts[14], counts[15]
void fe_launch_carry(hipStream_t s, const FeFrame& f);

// frontend_debug.hip: the Detections / Matches debug images (DESIGN.md 5.3 "Debug images"), BGR8 with dense rows (3 W bytes) into
// `bgr`, from the frame's record in `f` (status, kstar, seg, steps; the first n_out records of f.out) on stream s.
void fe_launch_debug_matches(hipStream_t s, const FeFrame& f, uint8_t* bgr);
void fe_launch_debug_detections(hipStream_t s, const FeFrame& f, int32_t n_out, uint8_t* bgr);

}  // namespace flamehip
