// tests/cpp/eval_facade.cc -- flame::Flame::update() with flame::GpuFrontEnd and Params::photo_error: the stat keys
// total_photo_error / avg_photo_error / photo_pixels, the front end's num_* keys, and Flame::getTruthStats.
// Compiles with the fallback types and with the cv:: / Eigen:: / Sophus:: stand-ins.
// Usage: eval_facade in.bin out.bin.  in.bin: int32 {W, H, frames, device, iterations, photo_error}, float32 {fx, fy, cx, cy,
// idepth_var_max_graph}, then per frame int32 {img_id, is_poseframe}, float32 {qx, qy, qz, qw, tx, ty, tz}, W x H grey bytes,
// W x H float32 true depths.
// out.bin, per frame: int32 {frame, update ok, bit k set = stat key k present (total_photo_error, avg_photo_error, photo_pixels),
// bit k set = timing key k present (photo_error, photo_error_device), n_vtx, truth ok}, float64 {total_photo_error,
// avg_photo_error, photo_pixels}, int64 stats {num_idepth_updates, num_fail_max_dropouts, num_fail_ambiguous_match,
// num_fail_max_cost, num_fail_max_var, num_fail_ref_patch_grad} (-1 = key not set), int64 flame_hip_frontend_info {ok, died,
// ambiguous, bad_match}, int64 {true_pos, true_neg, false_pos, false_neg}, float64 total_error, float32 {avg_error, precision,
// recall}; and when the update succeeded: idepths (n_vtx floats), the filtered idepth map and the truth error map (W x H floats
// each).  Prints one line per frame.  Exit code 0 = the last frame's update succeeded, 3 = it did not.
#include <cstdio>
#include <cstring>
#include <vector>

#include "flame/flame.h"
#include "flame/gpu_frontend.h"

static flame::SE3f make_pose(const float* q, const float* t) {
#ifdef FLAME_HAVE_SOPHUS
  return Sophus::SE3f(Eigen::Quaternionf(q[3], q[0], q[1], q[2]), Eigen::Vector3f(t[0], t[1], t[2]));
#else
  flame::SE3f p;
  for (int k = 0; k < 4; ++k) p.q[k] = q[k];
  for (int k = 0; k < 3; ++k) p.t[k] = t[k];
  return p;
#endif
}

static int64_t stat_or_minus1(const flame::utils::StatsTracker& s, const char* key) {
  return s.stats().count(key) ? static_cast<int64_t>(s.stats(key)) : -1;
}

int main(int argc, char** argv) {
  if (argc < 3) return 10;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 11;
  std::fseek(f, 0, SEEK_END);
  const long size = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<char> buf(static_cast<size_t>(size));
  const bool read_ok = std::fread(buf.data(), 1, buf.size(), f) == buf.size();
  std::fclose(f);
  if (!read_ok || buf.size() < 44) return 11;
  int32_t hdr[6];
  float k5[5];
  std::memcpy(hdr, buf.data(), 24);
  std::memcpy(k5, buf.data() + 24, 20);
  const int W = hdr[0], H = hdr[1], frames = hdr[2];
  const size_t npix = static_cast<size_t>(W) * H;

  flame::Params params;
  params.hip_device = hdr[3];
  params.nltgv2_iterations = hdr[4];
  params.photo_error = hdr[5] != 0;
  params.idepth_var_max_graph = k5[4];
  flame::Matrix3f K, Kinv;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K(r, c) = Kinv(r, c) = (r == c) ? 1.f : 0.f;
  K(0, 0) = k5[0]; K(1, 1) = k5[1]; K(0, 2) = k5[2]; K(1, 2) = k5[3];
  Kinv(0, 0) = 1.f / k5[0]; Kinv(1, 1) = 1.f / k5[1]; Kinv(0, 2) = -k5[2] / k5[0]; Kinv(1, 2) = -k5[3] / k5[1];
  flame::Flame sensor(W, H, K, Kinv, params);
  flame::GpuFrontEnd features(W, H, K, params);
  sensor.setFrontEnd(features.frontEnd());

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 12;
  const size_t rec = 8 + 28 + npix + 4 * npix;
  bool ok = false;
  flame::Image1b img(H, W);
  std::vector<float> depth(npix);
  for (int k = 0; k < frames; ++k) {
    const char* p = buf.data() + 44 + rec * k;
    if (p + rec > buf.data() + buf.size()) return 11;
    int32_t ih[2];
    float qt[7];
    std::memcpy(ih, p, 8);
    std::memcpy(qt, p + 8, 28);
    for (int y = 0; y < H; ++y) std::memcpy(img.ptr<uint8_t>(y), p + 36 + static_cast<size_t>(y) * W, W);
    std::memcpy(depth.data(), p + 36 + npix, 4 * npix);
    ok = sensor.update(0.1 * k, static_cast<uint32_t>(ih[0]), make_pose(qt, qt + 4), img, ih[1] != 0);
    const flame::utils::StatsTracker& st = sensor.stats();
    static const char* const kStat[3] = {"total_photo_error", "avg_photo_error", "photo_pixels"};
    static const char* const kTiming[2] = {"photo_error", "photo_error_device"};
    static const char* const kNum[6] = {"num_idepth_updates", "num_fail_max_dropouts", "num_fail_ambiguous_match", "num_fail_max_cost",
                                        "num_fail_max_var", "num_fail_ref_patch_grad"};
    static const char* const kInfo[4] = {"ok", "died", "ambiguous", "bad_match"};
    int32_t stat_bits = 0, timing_bits = 0;
    double photo[3];
    for (int i = 0; i < 3; ++i) { stat_bits |= st.stats().count(kStat[i]) ? 1 << i : 0; photo[i] = st.stats(kStat[i]); }
    for (int i = 0; i < 2; ++i) timing_bits |= st.timings().count(kTiming[i]) ? 1 << i : 0;
    int64_t num[6], info[4];
    for (int i = 0; i < 6; ++i) num[i] = stat_or_minus1(st, kNum[i]);
    for (int i = 0; i < 4; ++i)
      if (flame_hip_frontend_info(features.handle(), kInfo[i], &info[i])) info[i] = -2;
    std::vector<flame::Point2f> vtx;
    std::vector<float> idepths, map, err;
    flame::TruthStats ts;
    bool truth_ok = false;
    if (ok) {
      sensor.getInverseDepthMesh(&vtx, &idepths, nullptr, nullptr, nullptr, nullptr);
      if (!sensor.getFilteredInverseDepthMap(&map)) return 13;
      truth_ok = sensor.getTruthStats(depth, &ts, &err);
    }
    const int32_t h6[6] = {k, ok ? 1 : 0, stat_bits, timing_bits, static_cast<int32_t>(vtx.size()), truth_ok ? 1 : 0};
    std::fwrite(h6, 4, 6, out);
    std::fwrite(photo, 8, 3, out);
    std::fwrite(num, 8, 6, out);
    std::fwrite(info, 8, 4, out);
    const int64_t conf[4] = {ts.true_pos, ts.true_neg, ts.false_pos, ts.false_neg};
    std::fwrite(conf, 8, 4, out);
    std::fwrite(&ts.total_error, 8, 1, out);
    const float derived[3] = {ts.avg_error, ts.precision, ts.recall};
    std::fwrite(derived, 4, 3, out);
    if (ok) {
      std::fwrite(idepths.data(), 4, idepths.size(), out);
      std::fwrite(map.data(), 4, map.size(), out);
      if (!truth_ok) err.assign(npix, 0.f);
      std::fwrite(err.data(), 4, err.size(), out);
    }
    const int hip_error = features.lastError() ? features.lastError() : static_cast<int>(st.stats("hip_error"));
    std::printf("frame=%d update=%d hip_error=%d vtx=%d photo_keys=%d photo_pixels=%.0f total_photo_error=%.6f avg_photo_error=%.6f\n", k,
                ok ? 1 : 0, ok ? 0 : hip_error, static_cast<int>(vtx.size()), stat_bits, photo[2], photo[0], photo[1]);
  }
  std::fclose(out);
  return ok ? 0 : 3;
}
