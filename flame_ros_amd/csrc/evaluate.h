// flame_ros_amd/csrc/evaluate.h -- the evaluate stage: the pipeline's self-check.  Photometric error of a dense idepth map
// (the current image warped onto a comparison image) and the ground-truth confusion matrix of reference
// src/utils.cc:326-368 (getDepthConfusionMatrix).  Kernels: evaluate.hip; C ABI: flame_hip_photo_reference / _photo_error /
// _truth_stats (flame_hip.cpp); the statement: DESIGN.md 5.5, restated operation by operation in tests/eval_ref.py.
//
// Both kernels give results that are a function of the inputs alone, whatever the grid or the card: the photometric costs
// are integers (any reduction order gives the same bits); the truth stage's total_error is a sum of float32 errors in DOUBLE
// in a fixed shape that depends on W x H only -- block b owns pixels [1024 b, 1024 (b + 1)) and reduces them by one fixed
// tree into partial[b], and the caller adds the partials in ascending b.  (The reference sums float32 in row-major order,
// which no parallel kernel reproduces: this is the stage's one departure from it.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frontend.h"

namespace flamehip {

constexpr int kEvBlockPixels = 1024;  // pixels per block of both kernels (256 threads x 4)

inline int ev_num_blocks(int64_t npix) { return (int)((npix + kEvBlockPixels - 1) / kEvBlockPixels); }

// words[] of the photometric kernel (cleared by a memset the caller queues in front of the launch)
enum { kEvTotal256 = 0, kEvEvaluated = 1, kEvNoIdepth = 2, kEvBehind = 3, kEvOutside = 4, kEvPhotoWords = 5 };
// words[] of the truth kernel, likewise
enum { kEvTruePos = 0, kEvTrueNeg = 1, kEvFalsePos = 2, kEvFalseNeg = 3, kEvTruthWords = 4 };

struct EvPhoto {
  int32_t W, H;
  float fx, fy, cx, cy;
  FePose pose;                 // A = K R, c = K t of T_cmp_cur (frontend.h pose_record with Tc = T_world_cmp, Tr = T_world_cur)
  const float* idepth;         // W x H, NaN = none
  const uint8_t* cur;          // H rows of W bytes, dense
  const uint8_t* cmp;          // likewise
  unsigned long long* words;   // kEvPhotoWords
  float* err;                  // W x H or nullptr: D / 256, NaN where not evaluated
};

struct EvTruth {
  int64_t npix;
  const float* idepth;         // estimate, NaN = none
  const float* depth;          // truth, > 0 = there is truth
  unsigned long long* words;   // kEvTruthWords
  double* partial;             // ev_num_blocks(npix)
  float* err;                  // npix or nullptr
};

void ev_launch_photo(hipStream_t s, const EvPhoto& f);
void ev_launch_truth(hipStream_t s, const EvTruth& f);

}  // namespace flamehip
