// tests/cpp/predict_facade.cc -- flame::Flame::update() with Params::project_graph: a registered FrontEnd::track hands out
// synthetic features per frame (no images involved), do_nltgv2 = false, so the mesh hands out the x0 every frame started from.
// Compiles with the fallback types and with the cv:: / Eigen:: / Sophus:: stand-ins.
// Usage: predict_facade in.bin out.bin.  in.bin: int32 {W, H, frames, device, project_graph, init_with_prediction}, float32
// {fx, fy, cx, cy}, then per frame float32 {qx, qy, qz, qw, tx, ty, tz}, int32 n, n x float32 {x, y, mu, var}.
// out.bin, per frame whose update succeeded: int32 {frame, n_vtx, n_tris, predicted (-1 = stat not set), has_map}, vtx (2 n_vtx
// floats), idepths, triangles (3 n_tris int32), tri_validity (n_tris bytes), and the predicted map (W x H floats) when has_map.
// Prints one line per frame.  Exit code 0 = the last frame's update succeeded, 3 = it did not.
#include <cstdio>
#include <cstring>
#include <vector>

#include "flame/flame.h"

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
  if (!read_ok || buf.size() < 40) return 11;
  int32_t hdr[6];
  float k4[4];
  std::memcpy(hdr, buf.data(), 24);
  std::memcpy(k4, buf.data() + 24, 16);
  const int W = hdr[0], H = hdr[1], frames = hdr[2];

  flame::Params params;
  params.hip_device = hdr[3];
  params.project_graph = hdr[4] != 0;
  params.init_with_prediction = hdr[5] != 0;
  params.do_nltgv2 = false;
  flame::Matrix3f K, Kinv;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K(r, c) = Kinv(r, c) = (r == c) ? 1.f : 0.f;
  K(0, 0) = k4[0]; K(1, 1) = k4[1]; K(0, 2) = k4[2]; K(1, 2) = k4[3];
  Kinv(0, 0) = 1.f / k4[0]; Kinv(1, 1) = 1.f / k4[1]; Kinv(0, 2) = -k4[2] / k4[0]; Kinv(1, 2) = -k4[3] / k4[1];
  flame::Flame sensor(W, H, K, Kinv, params);

  const float* feats = nullptr;  // the frame in hand: n x {x, y, mu, var}
  int32_t n_feats = 0;
  flame::FrontEnd fe;
  fe.track = [&feats, &n_feats](const flame::FrameInput&, flame::FeatureSet* out) {
    out->vtx.resize(static_cast<size_t>(n_feats));
    out->idepth_mu.resize(static_cast<size_t>(n_feats));
    out->idepth_var.resize(static_cast<size_t>(n_feats));
    for (int32_t i = 0; i < n_feats; ++i) {
      out->vtx[i].x = feats[4 * i]; out->vtx[i].y = feats[4 * i + 1];
      out->idepth_mu[i] = feats[4 * i + 2]; out->idepth_var[i] = feats[4 * i + 3];
    }
    return true;
  };
  sensor.setFrontEnd(fe);

  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 12;
  bool ok = false;
  flame::Image1b img(H, W);
  const char* p = buf.data() + 40;
  const char* end = buf.data() + buf.size();
  std::vector<float> frame_feats;
  for (int k = 0; k < frames; ++k) {
    if (p + 32 > end) return 11;
    float qt[7];
    std::memcpy(qt, p, 28);
    std::memcpy(&n_feats, p + 28, 4);
    p += 32;
    if (n_feats < 0 || p + 16 * static_cast<size_t>(n_feats) > end) return 11;
    frame_feats.resize(4 * static_cast<size_t>(n_feats));
    std::memcpy(frame_feats.data(), p, 16 * static_cast<size_t>(n_feats));
    p += 16 * static_cast<size_t>(n_feats);
    feats = frame_feats.data();
    ok = sensor.update(0.1 * k, static_cast<uint32_t>(k), make_pose(qt, qt + 4), img, k == 0);
    const bool has_stage = sensor.stats().timings().count("project_graph") != 0;
    const int predicted = sensor.stats().stats().count("predicted") ? static_cast<int>(sensor.stats().stats("predicted")) : -1;
    std::vector<flame::Point2f> vtx;
    std::vector<float> idepths, map;
    std::vector<flame::Triangle> tris;
    std::vector<bool> valid;
    if (ok) {
      sensor.getInverseDepthMesh(&vtx, &idepths, nullptr, &tris, &valid, nullptr);
      const bool has_map = sensor.getPredictedInverseDepthMap(&map);
      const int32_t h5[5] = {k, static_cast<int32_t>(vtx.size()), static_cast<int32_t>(tris.size()), predicted, has_map ? 1 : 0};
      std::fwrite(h5, 4, 5, out);
      for (size_t i = 0; i < vtx.size(); ++i) { const float xy[2] = {vtx[i].x, vtx[i].y}; std::fwrite(xy, 4, 2, out); }
      std::fwrite(idepths.data(), 4, idepths.size(), out);
      for (size_t i = 0; i < tris.size(); ++i) { const int32_t abc[3] = {tris[i][0], tris[i][1], tris[i][2]}; std::fwrite(abc, 4, 3, out); }
      for (size_t i = 0; i < valid.size(); ++i) { const uint8_t b = valid[i] ? 1 : 0; std::fwrite(&b, 1, 1, out); }
      if (has_map) std::fwrite(map.data(), 4, map.size(), out);
    }
    std::printf("frame=%d update=%d hip_error=%d vtx=%d tris=%d project_graph=%d predicted=%d\n", k, ok ? 1 : 0,
                ok ? 0 : static_cast<int>(sensor.stats().stats("hip_error")), static_cast<int>(vtx.size()), static_cast<int>(tris.size()),
                has_stage ? 1 : 0, predicted);
  }
  std::fclose(out);
  return ok ? 0 : 3;
}
