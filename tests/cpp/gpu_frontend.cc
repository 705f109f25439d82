// tests/cpp/gpu_frontend.cc -- flame::Flame fed by flame::GpuFrontEnd (include/flame/gpu_frontend.h) through the plain
// update(time, img_id, pose, img, is_poseframe) overload, the call every flame_ros frontend makes (reference
// src/flame_offline_tum.cc:578-579).  Compiles with the fallback types and with the cv:: / Eigen:: / Sophus:: stand-ins.
// Usage: gpu_frontend in.bin out.bin.  in.bin: int32 {W, H, frames, device, iterations}, float32 {fx, fy, cx, cy}, then per
// frame int32 {img_id, is_poseframe}, float32 {qx, qy, qz, qw, tx, ty, tz}, W x H grey bytes.  Prints one line per frame;
// out.bin gets, for every frame whose update succeeded, int32 {frame, n_raw, n_vtx} + raw vtx / mu / var + mesh vtx / idepths.
// Exit code 0 = the last frame's update succeeded, 3 = it did not.
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
  if (!read_ok || buf.size() < 36) return 11;
  int32_t hdr[5];
  float k4[4];
  std::memcpy(hdr, buf.data(), 20);
  std::memcpy(k4, buf.data() + 20, 16);
  const int W = hdr[0], H = hdr[1], frames = hdr[2];

  flame::Params params;
  params.hip_device = hdr[3];
  params.nltgv2_iterations = hdr[4];
  flame::Matrix3f K, Kinv;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K(r, c) = Kinv(r, c) = (r == c) ? 1.f : 0.f;
  K(0, 0) = k4[0]; K(1, 1) = k4[1]; K(0, 2) = k4[2]; K(1, 2) = k4[3];
  Kinv(0, 0) = 1.f / k4[0]; Kinv(1, 1) = 1.f / k4[1]; Kinv(0, 2) = -k4[2] / k4[0]; Kinv(1, 2) = -k4[3] / k4[1];
  flame::Flame sensor(W, H, K, Kinv, params);
  flame::GpuFrontEnd features(W, H, K, params);
  sensor.setFrontEnd(features.frontEnd());

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 12;
  const size_t rec = 8 + 28 + static_cast<size_t>(W) * H;
  bool ok = false;
  flame::Image1b img(H, W);
  for (int k = 0; k < frames; ++k) {
    const char* p = buf.data() + 36 + rec * k;
    if (p + rec > buf.data() + buf.size()) return 11;
    int32_t ih[2];
    float qt[7];
    std::memcpy(ih, p, 8);
    std::memcpy(qt, p + 8, 28);
    for (int y = 0; y < H; ++y) std::memcpy(img.ptr<uint8_t>(y), p + 36 + static_cast<size_t>(y) * W, W);
    ok = sensor.update(0.1 * k, static_cast<uint32_t>(ih[0]), make_pose(qt, qt + 4), img, ih[1] != 0);
    std::vector<flame::Point2f> raw_vtx, vtx;
    std::vector<float> mu, var, idepths;
    std::vector<flame::Triangle> tris;
    if (ok) {
      sensor.getRawIDepths(&raw_vtx, &mu, &var);
      sensor.getInverseDepthMesh(&vtx, &idepths, nullptr, &tris, nullptr, nullptr);
      const int32_t h3[3] = {k, static_cast<int32_t>(raw_vtx.size()), static_cast<int32_t>(vtx.size())};
      std::fwrite(h3, 4, 3, out);
      for (size_t i = 0; i < raw_vtx.size(); ++i) { const float xy[2] = {raw_vtx[i].x, raw_vtx[i].y}; std::fwrite(xy, 4, 2, out); }
      std::fwrite(mu.data(), 4, mu.size(), out);
      std::fwrite(var.data(), 4, var.size(), out);
      for (size_t i = 0; i < vtx.size(); ++i) { const float xy[2] = {vtx[i].x, vtx[i].y}; std::fwrite(xy, 4, 2, out); }
      std::fwrite(idepths.data(), 4, idepths.size(), out);
    }
    // (Flame's own "hip_error" is the GPU tail's; a frame the front end failed carries its code in lastError())
    const int err = features.lastError() ? features.lastError() : static_cast<int>(sensor.stats().stats("hip_error"));
    std::printf("frame=%d update=%d hip_error=%d raw=%d vtx=%d tris=%d\n", k, ok ? 1 : 0, ok ? 0 : err, static_cast<int>(raw_vtx.size()),
                static_cast<int>(vtx.size()), static_cast<int>(tris.size()));
  }
  std::fclose(out);
  return ok ? 0 : 3;
}
