// flame_ros_amd/csrc/frontend.cpp -- C ABI of the feature front end (include/flame_hip.h, flame_hip_frontend_*): owns the
// pose-frame ring (images on the device, poses on the host in double), the feature slots and the per-frame scratch; a call
// of flame_hip_frontend_track uploads the image, queues kill -> track + project -> (detect) -> assign + compact on the
// handle's stream and returns when the emitted features are on the host.  Kernels: frontend.hip.  With a camera set
// (flame_hip_frontend_set_camera) flame_hip_frontend_track_raw puts the ingest stage (ingest.hip: grey, box downsample, undistort)
// between the upload of the raw image and the tracker, writing into the ring slot the tracker reads.  flame_hip_frontend_debug_image
// renders the Detections / Matches picture of the last tracked frame (frontend_debug.hip) from the record the tracker left on the
// device.  flame_hip_frontend_set_gates records the letterbox and the height band; every frame forms the gate record of FeFrame
// from them and the frame's pose.  flame_hip_frontend_set_cost records the matching cost (SSD / ZSSD); every frame forms the BAD_MATCH
// threshold of that cost and picks the tracker's instantiation; flame_hip_frontend_set_gain_invariant puts the gain-invariant cost in
// their place while it is on.  flame_hip_frontend_set_ref_grad records the reference-patch gradient
// gate; while it is on every frame forms the epipole table behind the pose table and runs the tracker's gated instantiation.
// flame_hip_frontend_set_warp records the warped-window switch; while it is on every frame runs the tracker's warped instantiation
// (it reads the pose table and the intrinsics the frame holds anyway).  flame_hip_frontend_set_carry records the hand-over switch;
// while it is on a pose frame that takes a ring slot in use goes into the extra image slot, no kill runs, k_fe_carry runs behind
// k_fe_compact and the image is copied into the ring slot on the stream.  Reads no environment variable.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/flame_hip.h"
#include "frontend.h"
#include "ingest.h"

using namespace flamehip;

struct flame_hip_frontend {
  int device = -1;
  int32_t W = 0, H = 0, max_features = 0, max_poseframes = 0;
  double fx = 0, fy = 0, cx = 0, cy = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t evi0 = nullptr, evi1 = nullptr;  // around the raw upload and the ingest stage
  // pose-frame ring (host side)
  std::vector<uint32_t> pf_id;
  std::vector<uint8_t> pf_used;
  std::vector<double> pf_T;  // 12 per slot: T_world_ref, row-major [R|t]
  int64_t pf_added = 0;
  // device
  uint8_t* d_imgs = nullptr;  // max_poseframes + 1 images
  FePose* d_poses = nullptr;
  char* d_state = nullptr;    // one arena for everything sized by max_features
  unsigned long long* d_cell_key = nullptr;
  int32_t* d_det = nullptr;
  int32_t cell_cap = 0;
  int32_t* d_counts = nullptr;
  FeFrame fr;  // the pointers, filled once
  // page-locked host staging
  uint8_t* h_img = nullptr;
  FePose* h_poses = nullptr;
  int32_t* h_counts = nullptr;
  FeOut* h_out = nullptr;
  // last frame
  int32_t n_out = 0;
  int32_t counts[kFeCounts] = {0};
  double track_us = 0.0, track_device_us = 0.0;
  bool timed = false;
  bool have_image = false;  // fr.cur holds the image the last track / track_raw call tracked
  // ingest stage (set_camera): raw image staging (page-locked host + device), the grey + box scratch, rectify's own output
  bool have_cam = false;
  InCam cam;
  size_t raw_cap = 0;  // bytes d_raw / h_raw hold
  uint8_t* h_raw = nullptr;
  uint8_t* d_raw = nullptr;
  uint8_t* d_scratch = nullptr;
  uint8_t* d_rect = nullptr;
  double ingest_device_us = 0.0;
  int64_t ingest_raw_bytes = 0;
  // debug images (flame_hip_frontend_debug_image): the rendered picture on the device and its page-locked copy, made at the first call
  uint8_t* d_dbg = nullptr;
  uint8_t* h_dbg = nullptr;
  double debug_image_device_us = 0.0;
  // gates (set_gates): all zero = none
  flame_hip_frontend_gates gates = {0, 0, 0.f, 0.f, {0.f, 0.f, 0.f}};
  // matching cost (set_cost): no state depends on it, so it may change between any two frames
  int32_t cost_mode = FLAME_HIP_FE_COST_SSD;
  // the gain-invariant cost (set_gain_invariant): while on it overrides cost_mode, which stays what set_cost set; no state either
  int32_t gain_invariant = 0;
  // the warped window (set_warp): no state depends on it either
  int32_t warp = 0;
  // the hand-over (set_carry): read by the evicting pose frames alone; no state depends on it either
  int32_t carry = 0;
  // reference-patch gradient gate (set_ref_grad): 0 = off; no state depends on it either
  float min_epi_grad = 0.f;
};

namespace {

inline int hip_err(hipError_t e) { return e == hipSuccess ? 0 : FLAME_HIP_ERR_HIP - (int)e; }
#define FE_HIP(x)                      \
  do {                                 \
    const hipError_t e_ = (x);         \
    if (e_ != hipSuccess) return hip_err(e_); \
  } while (0)

// the pose table and, behind it, the epipole table: one allocation on each side, one upload while the gradient gate is on
constexpr size_t kPoseBytes = sizeof(FePose) + sizeof(FeEpi);

template <class T>
T* carve(char*& p, size_t n) {
  T* r = reinterpret_cast<T*>(p);
  p += (n * sizeof(T) + 255) & ~(size_t)255;
  return r;
}

void release(flame_hip_frontend* fe) {
  if (fe->device >= 0) {
    (void)hipSetDevice(fe->device);
    if (fe->stream) (void)hipStreamSynchronize(fe->stream);
    if (fe->d_imgs) (void)hipFree(fe->d_imgs);
    if (fe->d_poses) (void)hipFree(fe->d_poses);
    if (fe->d_state) (void)hipFree(fe->d_state);
    if (fe->d_cell_key) (void)hipFree(fe->d_cell_key);
    if (fe->d_det) (void)hipFree(fe->d_det);
    if (fe->d_counts) (void)hipFree(fe->d_counts);
    if (fe->h_img) (void)hipHostFree(fe->h_img);
    if (fe->h_poses) (void)hipHostFree(fe->h_poses);
    if (fe->h_counts) (void)hipHostFree(fe->h_counts);
    if (fe->h_out) (void)hipHostFree(fe->h_out);
    if (fe->h_raw) (void)hipHostFree(fe->h_raw);
    if (fe->d_raw) (void)hipFree(fe->d_raw);
    if (fe->d_scratch) (void)hipFree(fe->d_scratch);
    if (fe->d_rect) (void)hipFree(fe->d_rect);
    if (fe->d_dbg) (void)hipFree(fe->d_dbg);
    if (fe->h_dbg) (void)hipHostFree(fe->h_dbg);
    if (fe->evi0) (void)hipEventDestroy(fe->evi0);
    if (fe->evi1) (void)hipEventDestroy(fe->evi1);
    if (fe->ev0) (void)hipEventDestroy(fe->ev0);
    if (fe->ev1) (void)hipEventDestroy(fe->ev1);
    if (fe->stream) (void)hipStreamDestroy(fe->stream);
  }
  delete fe;
}

bool finite12(const double* T) {
  for (int k = 0; k < 12; ++k)
    if (!std::isfinite(T[k])) return false;
  return true;
}

unsigned long long valid_mask(const flame_hip_frontend* fe) {
  unsigned long long m = 0;
  for (int p = 0; p < fe->max_poseframes; ++p)
    if (fe->pf_used[p]) m |= 1ull << p;
  return m;
}

int check_params(const flame_hip_frontend_params* p) {
  const float fl[] = {p->min_grad_mag, p->epipolar_line_var, p->idepth_min, p->idepth_max, p->idepth_init, p->var_init, p->max_match_error};
  for (float x : fl)
    if (!std::isfinite(x)) return FLAME_HIP_ERR_NAN;
  if (p->detection_win_size < 1 || p->win_size < 1 || p->win_size > kFeMaxWin || !(p->win_size & 1) || p->max_dropouts < 0 ||
      p->min_grad_mag < 0.f || p->min_grad_mag > 255.f || p->epipolar_line_var < 0.f || !(p->idepth_min < p->idepth_max) ||
      !(p->var_init > 0.f) || p->max_match_error < 0.f || p->max_match_error > 65025.f)
    return FLAME_HIP_ERR_ARG;
  return 0;
}

// the letterbox needs a band that holds a detection candidate's row with its window above and below
int check_band(const flame_hip_frontend* fe, const flame_hip_frontend_params* p) {
  if (!fe->gates.letterbox) return 0;
  const int32_t y_lo = fe->H / 3, y_hi = fe->H - fe->H / 3;
  return y_hi - y_lo < 2 * (p->win_size / 2 + 1) + 1 ? FLAME_HIP_ERR_ARG : 0;
}

// The frame's gate record: the band of rows, and hr = n^T R, h0 = n . t of T_world_cam = [R|t] in double (sums left to right),
// each rounded once to float32 (tests/fe_gates_ref.py gate_record() is the same statement).
FeGates gate_record(const flame_hip_frontend* fe, const double* T) {
  FeGates g;
  std::memset(&g, 0, sizeof(g));
  const flame_hip_frontend_gates& s = fe->gates;
  g.y_lo = s.letterbox ? fe->H / 3 : 0;
  g.y_hi = s.letterbox ? fe->H - fe->H / 3 : fe->H;
  g.height_gate = s.height_gate ? 1 : 0;
  if (g.height_gate) {
    const double n0 = s.up[0], n1 = s.up[1], n2 = s.up[2];
    g.min_height = s.min_height;
    g.max_height = s.max_height;
    g.hr0 = (float)((n0 * T[0] + n1 * T[4]) + n2 * T[8]);
    g.hr1 = (float)((n0 * T[1] + n1 * T[5]) + n2 * T[9]);
    g.hr2 = (float)((n0 * T[2] + n1 * T[6]) + n2 * T[10]);
    g.h0 = (float)((n0 * T[3] + n1 * T[7]) + n2 * T[11]);
  }
  return g;
}

// The BAD_MATCH threshold of a frame (DESIGN.md 5.3 "Matching cost"): bad = max_match_error win^2 65536 bounds the SSD cost; the
// ZSSD cost n S2 - S1^2 is bounded by n bad, saturated at UINT64_MAX (tests/fe_zm_ref.py bad_threshold() is the same statement), and
// so is the gain-invariant cost, whose unit is the same.  `cost` is the tracker's selector (kFeCost*).
uint64_t bad_threshold(float max_match_error, int32_t win, int cost) {
  const uint64_t n = (uint64_t)(win * win);
  const uint64_t bad = (uint64_t)((double)max_match_error * (double)(win * win) * 65536.0);
  if (cost == kFeCostSsd) return bad;
  return bad > UINT64_MAX / n ? UINT64_MAX : n * bad;
}

// the raw image, rows made dense, into the page-locked staging buffer
void stage_raw(flame_hip_frontend* fe, const uint8_t* raw, int32_t pitch) {
  const size_t row = (size_t)fe->cam.raw_w * in_channels(fe->cam.format);
  for (int32_t y = 0; y < fe->cam.raw_h; ++y) std::memcpy(fe->h_raw + (size_t)y * row, raw + (size_t)y * pitch, row);
}

// Queues the upload of the staged raw image and the ingest stage on the handle's stream (no synchronisation); `dst` gets the
// W x H rectified grey image.  The grey + box kernel is skipped for GRAY8 at resize factor 1, the remap when D is all zero.
int queue_ingest(flame_hip_frontend* fe, uint8_t* dst) {
  const InCam& c = fe->cam;
  hipStream_t s = fe->stream;
  const int32_t raw_pitch = c.raw_w * in_channels(c.format);
  const bool box = !(c.format == kInGray8 && c.f == 1);
  const bool remap = c.k1 != 0.f || c.k2 != 0.f || c.p1 != 0.f || c.p2 != 0.f || c.k3 != 0.f;
  FE_HIP(hipEventRecord(fe->evi0, s));
  uint8_t* up = (box || remap) ? fe->d_raw : dst;  // (nothing to do: the upload is the stage)
  FE_HIP(hipMemcpyAsync(up, fe->h_raw, (size_t)raw_pitch * c.raw_h, hipMemcpyHostToDevice, s));
  if (box) in_launch_grey_box(s, c, fe->d_raw, raw_pitch, remap ? fe->d_scratch : dst);
  if (remap) in_launch_remap(s, c, box ? fe->d_scratch : fe->d_raw, dst);
  FE_HIP(hipGetLastError());
  FE_HIP(hipEventRecord(fe->evi1, s));
  return 0;
}

}  // namespace

extern "C" {

void flame_hip_frontend_default_params(flame_hip_frontend_params* p) {
  if (!p) return;
  p->detection_win_size = 16;
  p->min_grad_mag = 5.0f;
  p->win_size = 5;
  p->epipolar_line_var = 4.0f;
  p->max_dropouts = 5;
  p->idepth_min = 0.01f;
  p->idepth_max = 10.0f;
  p->idepth_init = 0.5f;
  p->var_init = 0.25f;
  p->max_match_error = 100.0f;
}

int flame_hip_frontend_create(flame_hip_frontend** out, int device, int32_t W, int32_t H, const float K[9], int32_t max_features,
                              int32_t max_poseframes) {
  if (!out) return FLAME_HIP_ERR_ARG;
  *out = nullptr;
  if (!K || W < 8 || H < 8 || W > 8192 || H > 8192 || max_features < 1 || max_features > (1 << 22) || max_poseframes < 1 ||
      max_poseframes > kFeMaxPoseframes || device < -1)
    return FLAME_HIP_ERR_ARG;
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(K[k])) return FLAME_HIP_ERR_NAN;
  if (!(K[0] > 0.f) || !(K[4] > 0.f)) return FLAME_HIP_ERR_ARG;
  int n = 0;
  if (device >= 0 && (hipGetDeviceCount(&n) != hipSuccess || device >= n || hipSetDevice(device) != hipSuccess)) return FLAME_HIP_ERR_NODEVICE;
  flame_hip_frontend* fe = new (std::nothrow) flame_hip_frontend();
  if (!fe) return FLAME_HIP_ERR_ALLOC;
  fe->device = device;
  fe->W = W; fe->H = H; fe->max_features = max_features; fe->max_poseframes = max_poseframes;
  fe->fx = K[0]; fe->fy = K[4]; fe->cx = K[2]; fe->cy = K[5];
  fe->pf_id.assign(max_poseframes, 0);
  fe->pf_used.assign(max_poseframes, 0);
  fe->pf_T.assign(12 * (size_t)max_poseframes, 0.0);
  if (device < 0) {  // a handle without a device: arguments are checked, every call that needs the device returns NODEVICE
    std::memset(&fe->fr, 0, sizeof(fe->fr));
    *out = fe;
    return 0;
  }
  const size_t npix = (size_t)W * H, F = (size_t)max_features;
  const size_t state_bytes = 13 * ((F * 4 + 255) & ~(size_t)255) + ((F + 255) & ~(size_t)255) + 2 * ((F * sizeof(float4) + 255) & ~(size_t)255) +
                             ((F * sizeof(FeOut) + 255) & ~(size_t)255);
  bool ok = hipStreamCreateWithFlags(&fe->stream, hipStreamNonBlocking) == hipSuccess && hipEventCreate(&fe->ev0) == hipSuccess &&
            hipEventCreate(&fe->ev1) == hipSuccess && hipEventCreate(&fe->evi0) == hipSuccess && hipEventCreate(&fe->evi1) == hipSuccess;
  ok = ok && hipMalloc(&fe->d_imgs, npix * (size_t)(max_poseframes + 1)) == hipSuccess &&
       hipMalloc(&fe->d_poses, kPoseBytes * (size_t)max_poseframes) == hipSuccess && hipMalloc(&fe->d_state, state_bytes) == hipSuccess &&
       hipMalloc(&fe->d_counts, sizeof(int32_t) * kFeCounts) == hipSuccess &&
       hipHostMalloc(&fe->h_img, npix) == hipSuccess && hipHostMalloc(&fe->h_poses, kPoseBytes * (size_t)max_poseframes) == hipSuccess &&
       hipHostMalloc(&fe->h_counts, sizeof(int32_t) * kFeCounts) == hipSuccess && hipHostMalloc(&fe->h_out, sizeof(FeOut) * F) == hipSuccess;
  ok = ok && hipMemsetAsync(fe->d_state, 0, state_bytes, fe->stream) == hipSuccess &&
       hipMemsetAsync(fe->d_poses, 0, kPoseBytes * (size_t)max_poseframes, fe->stream) == hipSuccess &&
       hipStreamSynchronize(fe->stream) == hipSuccess;
  if (!ok) {
    release(fe);
    return FLAME_HIP_ERR_ALLOC;
  }
  FeFrame& f = fe->fr;
  std::memset(&f, 0, sizeof(f));
  char* p = fe->d_state;
  f.u = carve<int32_t>(p, F); f.v = carve<int32_t>(p, F); f.pf = carve<int32_t>(p, F); f.drop = carve<int32_t>(p, F);
  f.mu = carve<float>(p, F); f.var = carve<float>(p, F);
  f.status = carve<int32_t>(p, F); f.kstar = carve<int32_t>(p, F); f.cell_of = carve<int32_t>(p, F); f.freelist = carve<int32_t>(p, F);
  f.alive = carve<uint8_t>(p, F);
  f.proj = carve<float4>(p, F);
  f.out = carve<FeOut>(p, F);
  f.seg = carve<float4>(p, F);
  f.steps = carve<int32_t>(p, F);
  f.W = W; f.H = H; f.max_features = max_features;
  f.fx = K[0]; f.fy = K[4]; f.cx = K[2]; f.cy = K[5];
  f.imgs = fe->d_imgs;
  f.poses = fe->d_poses;
  f.epi = reinterpret_cast<const FeEpi*>(fe->d_poses + max_poseframes);
  f.counts = fe->d_counts;
  *out = fe;
  return 0;
}

void flame_hip_frontend_destroy(flame_hip_frontend* fe) {
  if (fe) release(fe);
}

// One frame (flame_hip_frontend_track / _track_raw, arguments checked by the caller): `raw` = the image goes through the ingest
// stage of the handle's camera on its way into the ring slot, otherwise it is uploaded there as it is.
static int run_track(flame_hip_frontend* fe, const flame_hip_frontend_params* params, const uint8_t* img, int32_t pitch, bool raw,
                     uint32_t img_id, const double T_world_cam[12], int32_t is_poseframe, int32_t* n_out) {
  const auto t0 = std::chrono::steady_clock::now();
  FE_HIP(hipSetDevice(fe->device));
  const int32_t W = fe->W, H = fe->H;
  const size_t npix = (size_t)W * H;
  FeFrame& f = fe->fr;
  f.win = params->win_size;
  f.dws = params->detection_win_size;
  f.ncx = (W + f.dws - 1) / f.dws;
  f.ncy = (H + f.dws - 1) / f.dws;
  f.max_dropouts = params->max_dropouts;
  {
    const double g = std::ceil(4.0 * (double)params->min_grad_mag * (double)params->min_grad_mag);
    f.g2_min = g < 1.0 ? 1 : (int32_t)g;
  }
  f.idepth_min = params->idepth_min; f.idepth_max = params->idepth_max;
  f.idepth_init = params->idepth_init; f.var_init = params->var_init;
  f.epipolar_line_var = params->epipolar_line_var;
  const int cost = fe->gain_invariant ? kFeCostGi : fe->cost_mode == FLAME_HIP_FE_COST_ZSSD ? kFeCostZssd : kFeCostSsd;
  f.bad_match_cost = bad_threshold(params->max_match_error, f.win, cost);
  const bool ref_grad = fe->min_epi_grad > 0.f;
  f.min_epi_grad = fe->min_epi_grad;
  f.is_poseframe = is_poseframe ? 1 : 0;
  f.gates = gate_record(fe, T_world_cam);
  const int32_t ncells = f.ncx * f.ncy;
  if (ncells > fe->cell_cap) {  // (grows with the smallest cell size seen; bounded by the image)
    FE_HIP(hipStreamSynchronize(fe->stream));
    if (fe->d_cell_key) (void)hipFree(fe->d_cell_key);
    if (fe->d_det) (void)hipFree(fe->d_det);
    fe->d_cell_key = nullptr; fe->d_det = nullptr; fe->cell_cap = 0;
    FE_HIP(hipMalloc(&fe->d_cell_key, (sizeof(unsigned long long) + sizeof(int32_t)) * (size_t)ncells));  // the keys, then the held flags
    FE_HIP(hipMalloc(&fe->d_det, sizeof(int32_t) * (size_t)ncells));
    fe->cell_cap = ncells;
    f.cell_key = fe->d_cell_key;
    f.det = fe->d_det;
  }
  f.cell_held = reinterpret_cast<int32_t*>(fe->d_cell_key + ncells);  // (behind this frame's keys: one clear covers both)
  // a pose frame takes the ring's next slot; the features of the pose frame it overwrites die before tracking -- or, with the
  // hand-over on (DESIGN.md 5.3 "Hand-over"), are tracked against the new image once more: the image goes into the extra slot, the
  // ring slot keeps the old pose frame's image and record through the frame, and k_fe_carry hands the emitted ones over
  int32_t cur = fe->max_poseframes;  // the extra image slot
  int32_t img_slot = cur;            // where this frame's image goes
  bool overwrote = false, carry = false;
  if (is_poseframe) {
    cur = (int32_t)(fe->pf_added % fe->max_poseframes);
    overwrote = fe->pf_used[cur] != 0;
    carry = overwrote && fe->carry != 0;
    if (carry) overwrote = false;
    else { fe->pf_used[cur] = 0; img_slot = cur; }
  }
  uint8_t* const d_cur = fe->d_imgs + (size_t)img_slot * npix;
  f.cur_pf = cur;
  f.cur = d_cur;
  for (int p = 0; p < fe->max_poseframes; ++p) {
    if (fe->pf_used[p]) pose_record(fe->fx, fe->fy, fe->cx, fe->cy, T_world_cam, &fe->pf_T[12 * (size_t)p], &fe->h_poses[p]);
    else std::memset(&fe->h_poses[p], 0, sizeof(FePose));
  }
  if (ref_grad) {
    FeEpi* h_epi = reinterpret_cast<FeEpi*>(fe->h_poses + fe->max_poseframes);
    for (int p = 0; p < fe->max_poseframes; ++p) {
      if (fe->pf_used[p]) epipole_record(fe->fx, fe->fy, fe->cx, fe->cy, T_world_cam, &fe->pf_T[12 * (size_t)p], &h_epi[p]);
      else std::memset(&h_epi[p], 0, sizeof(FeEpi));
    }
  }
  hipStream_t s = fe->stream;
  if (raw) {
    stage_raw(fe, img, pitch);
    FE_HIP(hipEventRecord(fe->ev0, s));
    if (const int rc = queue_ingest(fe, d_cur)) return rc;
  } else {
    for (int32_t y = 0; y < H; ++y) std::memcpy(fe->h_img + (size_t)y * W, img + (size_t)y * pitch, (size_t)W);
    FE_HIP(hipEventRecord(fe->ev0, s));
    FE_HIP(hipMemcpyAsync(d_cur, fe->h_img, npix, hipMemcpyHostToDevice, s));
  }
  FE_HIP(hipMemcpyAsync(fe->d_poses, fe->h_poses, (ref_grad ? kPoseBytes : sizeof(FePose)) * (size_t)fe->max_poseframes, hipMemcpyHostToDevice, s));
  FE_HIP(hipMemsetAsync(fe->d_cell_key, 0xFF, (sizeof(unsigned long long) + sizeof(int32_t)) * (size_t)ncells, s));
  FE_HIP(hipMemsetAsync(fe->d_counts, 0, sizeof(int32_t) * kFeCounts, s));
  if (overwrote) fe_launch_kill(s, f, valid_mask(fe));
  fe_launch_track(s, f, cost, ref_grad, fe->warp != 0);
  if (is_poseframe) fe_launch_detect(s, f);
  fe_launch_compact(s, f);
  if (carry) {  // the old pose frame's emitted features move to the new one, the rest of them die; then the ring slot takes the image
    fe_launch_carry(s, f);
    FE_HIP(hipGetLastError());
    FE_HIP(hipMemcpyAsync(fe->d_imgs + (size_t)cur * npix, d_cur, npix, hipMemcpyDeviceToDevice, s));
    f.cur = fe->d_imgs + (size_t)cur * npix;  // (the same bytes: the extra slot is free again)
  }
  FE_HIP(hipGetLastError());
  FE_HIP(hipMemcpyAsync(fe->h_counts, fe->d_counts, sizeof(int32_t) * kFeCounts, hipMemcpyDeviceToHost, s));
  FE_HIP(hipEventRecord(fe->ev1, s));
  FE_HIP(hipStreamSynchronize(s));
  std::memcpy(fe->counts, fe->h_counts, sizeof(fe->counts));
  fe->n_out = fe->counts[0];
  if (fe->n_out < 0 || fe->n_out > fe->max_features) return FLAME_HIP_ERR_STATE;
  if (fe->n_out > 0) {
    FE_HIP(hipMemcpyAsync(fe->h_out, f.out, sizeof(FeOut) * (size_t)fe->n_out, hipMemcpyDeviceToHost, s));
    FE_HIP(hipStreamSynchronize(s));
  }
  if (is_poseframe) {  // the ring slot is valid from now on
    fe->pf_used[cur] = 1;
    fe->pf_id[cur] = img_id;
    std::memcpy(&fe->pf_T[12 * (size_t)cur], T_world_cam, 12 * sizeof(double));
    ++fe->pf_added;
  }
  fe->have_image = true;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, fe->ev0, fe->ev1) == hipSuccess) fe->track_device_us = 1000.0 * ms;
  fe->ingest_device_us = 0.0;
  fe->ingest_raw_bytes = 0;
  if (raw) {
    if (hipEventElapsedTime(&ms, fe->evi0, fe->evi1) == hipSuccess) fe->ingest_device_us = 1000.0 * ms;
    fe->ingest_raw_bytes = (int64_t)fe->cam.raw_h * fe->cam.raw_w * in_channels(fe->cam.format);
  }
  fe->track_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  *n_out = fe->n_out;
  return 0;
}

int flame_hip_frontend_track(flame_hip_frontend* fe, const flame_hip_frontend_params* params, const uint8_t* img, int32_t pitch,
                             uint32_t img_id, const double T_world_cam[12], int32_t is_poseframe, int32_t* n_out) {
  if (!fe || !params || !img || !T_world_cam || !n_out || pitch < fe->W) return FLAME_HIP_ERR_ARG;
  *n_out = 0;
  if (const int rc = check_params(params)) return rc;
  if (!finite12(T_world_cam)) return FLAME_HIP_ERR_NAN;
  if (const int rc = check_band(fe, params)) return rc;
  if (fe->device < 0) return FLAME_HIP_ERR_NODEVICE;
  return run_track(fe, params, img, pitch, false, img_id, T_world_cam, is_poseframe, n_out);
}

int flame_hip_frontend_set_camera(flame_hip_frontend* fe, const flame_hip_camera* cam) {
  if (!fe) return FLAME_HIP_ERR_ARG;
  if (!cam) {  // back to rectified input (the staging stays for the next camera)
    fe->have_cam = false;
    return 0;
  }
  if (cam->format < 0 || cam->format >= kInFormats || cam->resize_factor < 1 || cam->resize_factor > kInMaxResize || cam->raw_width < 1 ||
      cam->raw_height < 1 || cam->raw_width / cam->resize_factor != fe->W || cam->raw_height / cam->resize_factor != fe->H)
    return FLAME_HIP_ERR_ARG;
  for (int k = 0; k < 5; ++k)
    if (!std::isfinite(cam->D[k])) return FLAME_HIP_ERR_NAN;
  InCam c;
  c.raw_w = cam->raw_width; c.raw_h = cam->raw_height; c.format = cam->format; c.f = cam->resize_factor;
  c.W = fe->W; c.H = fe->H;
  c.fx = (float)fe->fx; c.fy = (float)fe->fy; c.cx = (float)fe->cx; c.cy = (float)fe->cy;
  c.k1 = cam->D[0]; c.k2 = cam->D[1]; c.p1 = cam->D[2]; c.p2 = cam->D[3]; c.k3 = cam->D[4];
  if (fe->device >= 0) {
    FE_HIP(hipSetDevice(fe->device));
    FE_HIP(hipStreamSynchronize(fe->stream));
    const size_t need = (size_t)c.raw_h * c.raw_w * in_channels(c.format), npix = (size_t)fe->W * fe->H;
    if (need > fe->raw_cap) {
      fe->have_cam = false;
      if (fe->h_raw) (void)hipHostFree(fe->h_raw);
      if (fe->d_raw) (void)hipFree(fe->d_raw);
      fe->h_raw = nullptr; fe->d_raw = nullptr; fe->raw_cap = 0;
      if (hipHostMalloc(&fe->h_raw, need) != hipSuccess || hipMalloc(&fe->d_raw, need) != hipSuccess) return FLAME_HIP_ERR_ALLOC;
      fe->raw_cap = need;
    }
    if (!fe->d_scratch && hipMalloc(&fe->d_scratch, npix) != hipSuccess) return FLAME_HIP_ERR_ALLOC;
    if (!fe->d_rect && hipMalloc(&fe->d_rect, npix) != hipSuccess) return FLAME_HIP_ERR_ALLOC;
  }
  fe->cam = c;
  fe->have_cam = true;
  return 0;
}

int flame_hip_frontend_set_gates(flame_hip_frontend* fe, const flame_hip_frontend_gates* gates) {
  if (!fe) return FLAME_HIP_ERR_ARG;
  flame_hip_frontend_gates g = {0, 0, 0.f, 0.f, {0.f, 0.f, 0.f}};
  if (gates) {
    g.letterbox = gates->letterbox ? 1 : 0;
    if (gates->height_gate) {  // (the band and the up vector are read only with the gate on)
      const float fl[] = {gates->min_height, gates->max_height, gates->up[0], gates->up[1], gates->up[2]};
      for (float x : fl)
        if (!std::isfinite(x)) return FLAME_HIP_ERR_NAN;
      if (gates->min_height > gates->max_height || (gates->up[0] == 0.f && gates->up[1] == 0.f && gates->up[2] == 0.f)) return FLAME_HIP_ERR_ARG;
      g.height_gate = 1;
      g.min_height = gates->min_height; g.max_height = gates->max_height;
      for (int k = 0; k < 3; ++k) g.up[k] = gates->up[k];
    }
  }
  fe->gates = g;  // takes effect with the next frame
  return 0;
}

int flame_hip_frontend_set_cost(flame_hip_frontend* fe, int32_t mode) {
  if (!fe || (mode != FLAME_HIP_FE_COST_SSD && mode != FLAME_HIP_FE_COST_ZSSD)) return FLAME_HIP_ERR_ARG;
  fe->cost_mode = mode;  // takes effect with the next frame
  return 0;
}

int flame_hip_frontend_set_gain_invariant(flame_hip_frontend* fe, int32_t on) {
  if (!fe || (on != 0 && on != 1)) return FLAME_HIP_ERR_ARG;
  fe->gain_invariant = on;  // takes effect with the next frame; cost_mode stays what set_cost set
  return 0;
}

int flame_hip_frontend_set_warp(flame_hip_frontend* fe, int32_t on) {
  if (!fe || (on != 0 && on != 1)) return FLAME_HIP_ERR_ARG;
  fe->warp = on;  // takes effect with the next frame
  return 0;
}

int flame_hip_frontend_set_carry(flame_hip_frontend* fe, int32_t on) {
  if (!fe || (on != 0 && on != 1)) return FLAME_HIP_ERR_ARG;
  fe->carry = on;  // takes effect with the next pose frame that takes a ring slot in use
  return 0;
}

int flame_hip_frontend_set_ref_grad(flame_hip_frontend* fe, float min_grad) {
  if (!fe) return FLAME_HIP_ERR_ARG;
  if (!std::isfinite(min_grad)) return FLAME_HIP_ERR_NAN;
  if (min_grad < 0.f) return FLAME_HIP_ERR_ARG;
  fe->min_epi_grad = min_grad;  // takes effect with the next frame; 0 = off
  return 0;
}

int flame_hip_frontend_track_raw(flame_hip_frontend* fe, const flame_hip_frontend_params* params, const uint8_t* raw, int32_t pitch,
                                 uint32_t img_id, const double T_world_cam[12], int32_t is_poseframe, int32_t* n_out) {
  if (!fe || !params || !raw || !T_world_cam || !n_out) return FLAME_HIP_ERR_ARG;
  *n_out = 0;
  if (!fe->have_cam) return FLAME_HIP_ERR_STATE;
  if (pitch < fe->cam.raw_w * in_channels(fe->cam.format)) return FLAME_HIP_ERR_ARG;
  if (const int rc = check_params(params)) return rc;
  if (!finite12(T_world_cam)) return FLAME_HIP_ERR_NAN;
  if (const int rc = check_band(fe, params)) return rc;
  if (fe->device < 0) return FLAME_HIP_ERR_NODEVICE;
  return run_track(fe, params, raw, pitch, true, img_id, T_world_cam, is_poseframe, n_out);
}

int flame_hip_frontend_rectify(flame_hip_frontend* fe, const uint8_t* raw, int32_t pitch, uint8_t* out, int32_t out_pitch) {
  if (!fe || !raw || !out || out_pitch < fe->W) return FLAME_HIP_ERR_ARG;
  if (!fe->have_cam) return FLAME_HIP_ERR_STATE;
  if (pitch < fe->cam.raw_w * in_channels(fe->cam.format)) return FLAME_HIP_ERR_ARG;
  if (fe->device < 0) return FLAME_HIP_ERR_NODEVICE;
  FE_HIP(hipSetDevice(fe->device));
  const size_t npix = (size_t)fe->W * fe->H;
  stage_raw(fe, raw, pitch);
  if (const int rc = queue_ingest(fe, fe->d_rect)) return rc;
  FE_HIP(hipMemcpyAsync(fe->h_img, fe->d_rect, npix, hipMemcpyDeviceToHost, fe->stream));
  FE_HIP(hipStreamSynchronize(fe->stream));
  for (int32_t y = 0; y < fe->H; ++y) std::memcpy(out + (size_t)y * out_pitch, fe->h_img + (size_t)y * fe->W, (size_t)fe->W);
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, fe->evi0, fe->evi1) == hipSuccess) fe->ingest_device_us = 1000.0 * ms;
  fe->ingest_raw_bytes = (int64_t)fe->cam.raw_h * fe->cam.raw_w * in_channels(fe->cam.format);
  return 0;
}

int flame_hip_frontend_image(flame_hip_frontend* fe, uint8_t* out, int32_t out_pitch) {
  if (!fe || !out || out_pitch < fe->W) return FLAME_HIP_ERR_ARG;
  if (fe->device < 0) return FLAME_HIP_ERR_NODEVICE;
  if (!fe->have_image) return FLAME_HIP_ERR_STATE;
  FE_HIP(hipSetDevice(fe->device));
  const size_t npix = (size_t)fe->W * fe->H;
  FE_HIP(hipMemcpyAsync(fe->h_img, fe->fr.cur, npix, hipMemcpyDeviceToHost, fe->stream));
  FE_HIP(hipStreamSynchronize(fe->stream));
  for (int32_t y = 0; y < fe->H; ++y) std::memcpy(out + (size_t)y * out_pitch, fe->h_img + (size_t)y * fe->W, (size_t)fe->W);
  return 0;
}

int flame_hip_frontend_features(flame_hip_frontend* fe, int32_t cap, float* vtx, float* idepth_mu, float* idepth_var, int32_t* slot,
                                int32_t* status) {
  if (!fe || cap < fe->n_out) return FLAME_HIP_ERR_ARG;
  for (int32_t i = 0; i < fe->n_out; ++i) {
    const FeOut& o = fe->h_out[i];
    if (vtx) { vtx[2 * i] = o.x; vtx[2 * i + 1] = o.y; }
    if (idepth_mu) idepth_mu[i] = o.mu;
    if (idepth_var) idepth_var[i] = o.var;
    if (slot) slot[i] = o.slot;
    if (status) status[i] = o.status;
  }
  return 0;
}

int flame_hip_frontend_set_poses(flame_hip_frontend* fe, int32_t n, const uint32_t* ids, const double* T) {
  if (!fe || n < 0 || (n > 0 && (!ids || !T))) return FLAME_HIP_ERR_ARG;
  for (int32_t i = 0; i < n; ++i)
    if (!finite12(T + 12 * (size_t)i)) return FLAME_HIP_ERR_NAN;
  for (int32_t i = 0; i < n; ++i)
    for (int p = 0; p < fe->max_poseframes; ++p)
      if (fe->pf_used[p] && fe->pf_id[p] == ids[i]) std::memcpy(&fe->pf_T[12 * (size_t)p], T + 12 * (size_t)i, 12 * sizeof(double));
  return 0;  // (an id the ring no longer holds is ignored: the caller's window may be longer than the ring)
}

int flame_hip_frontend_prune(flame_hip_frontend* fe, int32_t n, const uint32_t* keep_ids) {
  if (!fe || n < 0 || (n > 0 && !keep_ids)) return FLAME_HIP_ERR_ARG;
  bool dropped = false;
  for (int p = 0; p < fe->max_poseframes; ++p) {
    if (!fe->pf_used[p]) continue;
    bool keep = false;
    for (int32_t i = 0; i < n; ++i) keep = keep || keep_ids[i] == fe->pf_id[p];
    if (!keep) { fe->pf_used[p] = 0; dropped = true; }
  }
  if (dropped) {
    if (fe->device < 0) return FLAME_HIP_ERR_NODEVICE;
    FE_HIP(hipSetDevice(fe->device));
    fe_launch_kill(fe->stream, fe->fr, valid_mask(fe));
    FE_HIP(hipGetLastError());
    FE_HIP(hipStreamSynchronize(fe->stream));
  }
  return 0;
}

int flame_hip_frontend_state(flame_hip_frontend* fe, uint8_t* alive, int32_t* u, int32_t* v, int32_t* poseframe, float* mu, float* var,
                             int32_t* dropouts, int32_t* status, int32_t* kstar) {
  if (!fe) return FLAME_HIP_ERR_ARG;
  if (fe->device < 0) return FLAME_HIP_ERR_NODEVICE;
  FE_HIP(hipSetDevice(fe->device));
  FE_HIP(hipStreamSynchronize(fe->stream));
  const size_t F = (size_t)fe->max_features;
  const FeFrame& f = fe->fr;
  if (alive) FE_HIP(hipMemcpy(alive, f.alive, F, hipMemcpyDeviceToHost));
  if (u) FE_HIP(hipMemcpy(u, f.u, 4 * F, hipMemcpyDeviceToHost));
  if (v) FE_HIP(hipMemcpy(v, f.v, 4 * F, hipMemcpyDeviceToHost));
  if (poseframe) FE_HIP(hipMemcpy(poseframe, f.pf, 4 * F, hipMemcpyDeviceToHost));
  if (mu) FE_HIP(hipMemcpy(mu, f.mu, 4 * F, hipMemcpyDeviceToHost));
  if (var) FE_HIP(hipMemcpy(var, f.var, 4 * F, hipMemcpyDeviceToHost));
  if (dropouts) FE_HIP(hipMemcpy(dropouts, f.drop, 4 * F, hipMemcpyDeviceToHost));
  if (status) FE_HIP(hipMemcpy(status, f.status, 4 * F, hipMemcpyDeviceToHost));
  if (kstar) FE_HIP(hipMemcpy(kstar, f.kstar, 4 * F, hipMemcpyDeviceToHost));
  return 0;
}

int flame_hip_frontend_searches(flame_hip_frontend* fe, float* seg, int32_t* steps) {
  if (!fe) return FLAME_HIP_ERR_ARG;
  if (fe->device < 0) return FLAME_HIP_ERR_NODEVICE;
  if (!fe->have_image) return FLAME_HIP_ERR_STATE;
  FE_HIP(hipSetDevice(fe->device));
  FE_HIP(hipStreamSynchronize(fe->stream));
  const size_t F = (size_t)fe->max_features;
  if (seg) FE_HIP(hipMemcpy(seg, fe->fr.seg, 16 * F, hipMemcpyDeviceToHost));
  if (steps) FE_HIP(hipMemcpy(steps, fe->fr.steps, 4 * F, hipMemcpyDeviceToHost));
  return 0;
}

int flame_hip_frontend_debug_image(flame_hip_frontend* fe, int32_t kind, uint8_t* bgr, int32_t pitch) {
  if (!fe || !bgr || (kind != FLAME_HIP_FE_IMG_DETECTIONS && kind != FLAME_HIP_FE_IMG_MATCHES) || pitch < 3 * fe->W) return FLAME_HIP_ERR_ARG;
  if (fe->device < 0) return FLAME_HIP_ERR_NODEVICE;
  if (!fe->have_image) return FLAME_HIP_ERR_STATE;
  FE_HIP(hipSetDevice(fe->device));
  const size_t row = 3 * (size_t)fe->W, bytes = row * fe->H;
  if (!fe->d_dbg && hipMalloc(&fe->d_dbg, bytes) != hipSuccess) return FLAME_HIP_ERR_ALLOC;
  if (!fe->h_dbg && hipHostMalloc(&fe->h_dbg, bytes) != hipSuccess) return FLAME_HIP_ERR_ALLOC;
  hipStream_t s = fe->stream;
  FE_HIP(hipEventRecord(fe->ev0, s));
  if (kind == FLAME_HIP_FE_IMG_MATCHES) fe_launch_debug_matches(s, fe->fr, fe->d_dbg);
  else fe_launch_debug_detections(s, fe->fr, fe->n_out, fe->d_dbg);
  FE_HIP(hipGetLastError());
  FE_HIP(hipEventRecord(fe->ev1, s));
  FE_HIP(hipMemcpyAsync(fe->h_dbg, fe->d_dbg, bytes, hipMemcpyDeviceToHost, s));
  FE_HIP(hipStreamSynchronize(s));
  for (int32_t y = 0; y < fe->H; ++y) std::memcpy(bgr + (size_t)y * pitch, fe->h_dbg + (size_t)y * row, row);
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, fe->ev0, fe->ev1) == hipSuccess) fe->debug_image_device_us = 1000.0 * ms;
  return 0;
}

int flame_hip_frontend_info(flame_hip_frontend* fe, const char* key, int64_t* value) {
  if (!fe || !key || !value) return FLAME_HIP_ERR_ARG;
  static const char* const kStatus[] = {"ok", "no_parallax", "outside", "bad_match", "ambiguous", "new", "died"};
  for (int k = 0; k < 7; ++k)
    if (!std::strcmp(key, kStatus[k])) { *value = fe->counts[2 + k]; return 0; }
  if (!std::strcmp(key, "emitted")) { *value = fe->n_out; return 0; }
  if (!std::strcmp(key, "detections_dropped")) { *value = fe->counts[9]; return 0; }
  if (!std::strcmp(key, "track_us")) { *value = (int64_t)(fe->track_us + 0.5); return 0; }
  if (!std::strcmp(key, "track_device_us")) { *value = (int64_t)(fe->track_device_us + 0.5); return 0; }
  if (!std::strcmp(key, "max_features")) { *value = fe->max_features; return 0; }
  if (!std::strcmp(key, "ingest_device_us")) { *value = (int64_t)(fe->ingest_device_us + 0.5); return 0; }
  if (!std::strcmp(key, "ingest_raw_bytes")) { *value = fe->ingest_raw_bytes; return 0; }
  if (!std::strcmp(key, "debug_image_device_us")) { *value = (int64_t)(fe->debug_image_device_us + 0.5); return 0; }
  if (!std::strcmp(key, "gates")) { *value = (fe->gates.letterbox ? 1 : 0) | (fe->gates.height_gate ? 2 : 0); return 0; }
  if (!std::strcmp(key, "cost_mode")) { *value = fe->cost_mode; return 0; }
  if (!std::strcmp(key, "gain_invariant")) { *value = fe->gain_invariant; return 0; }
  if (!std::strcmp(key, "warp")) { *value = fe->warp; return 0; }
  if (!std::strcmp(key, "warp_refused")) { *value = fe->counts[13]; return 0; }
  if (!std::strcmp(key, "carry")) { *value = fe->carry; return 0; }
  if (!std::strcmp(key, "carried")) { *value = fe->counts[14]; return 0; }
  if (!std::strcmp(key, "carry_lost")) { *value = fe->counts[15]; return 0; }
  if (!std::strcmp(key, "ref_grad")) { *value = fe->min_epi_grad > 0.f ? 1 : 0; return 0; }
  if (!std::strcmp(key, "fail_ref_grad")) { *value = fe->counts[12]; return 0; }
  if (!std::strcmp(key, "held_height")) { *value = fe->counts[10]; return 0; }
  if (!std::strcmp(key, "refused_letterbox")) { *value = fe->counts[11]; return 0; }
  if (!std::strcmp(key, "camera")) { *value = fe->have_cam ? 1 : 0; return 0; }
  if (!std::strcmp(key, "poseframes")) {
    int64_t c = 0;
    for (int p = 0; p < fe->max_poseframes; ++p) c += fe->pf_used[p] ? 1 : 0;
    *value = c;
    return 0;
  }
  if (!std::strcmp(key, "live")) {  // counted where the state lives (a prune since the last frame shows)
    std::vector<uint8_t> a((size_t)fe->max_features);
    if (const int rc = flame_hip_frontend_state(fe, a.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)) return rc;
    int64_t c = 0;
    for (uint8_t x : a) c += x ? 1 : 0;
    *value = c;
    return 0;
  }
  return FLAME_HIP_ERR_ARG;
}

}  // extern "C"
