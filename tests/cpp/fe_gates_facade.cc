// tests/cpp/fe_gates_facade.cc -- the front end's gates behind flame::GpuFrontEnd (Params::do_letterbox, min_height / max_height,
// setUpAxis / setGates): three Flame + front-end pairs over one sequence of grey frames --
//   G: Params::do_letterbox and a finite Params::min_height (default up axis);
//   U: the reference's defaults (no gate);
//   P: the reference's defaults, the FrontEnd's `track` written here on a handle of its own with flame_hip_frontend_track /
//      _features alone -- a pair built without any call of the gates.
// After every update(): every mesh vertex of G lies in the letterbox rows, G's stats carry num_held_height /
// num_refused_letterbox (U's do not), and U's mesh equals P's byte for byte.  Before the frames, on a handle without a device
// (hip_device = -1): a band the library refuses lands in lastError() and fails track(); setGates() repairs it.
// Compiles with the fallback types and with the cv:: / Eigen:: / Sophus:: stand-ins.
// Usage: fe_gates_facade in.bin.  in.bin: int32 {W, H, frames, device, iterations}, float32 {fx, fy, cx, cy, min_height}, then per
// frame int32 {img_id, is_poseframe}, float32 {qx, qy, qz, qw, tx, ty, tz}, W x H grey bytes.  One line per frame; exit code 0 =
// every check held and the last updates succeeded, 3 = a last update failed, 4 = a check failed.
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

struct Mesh {
  std::vector<flame::Point2f> vtx;
  std::vector<float> idepths;
};
static Mesh mesh_of(const flame::Flame& sensor) {
  Mesh m;
  sensor.getInverseDepthMesh(&m.vtx, &m.idepths, nullptr, nullptr, nullptr, nullptr);
  return m;
}
static bool same(const Mesh& a, const Mesh& b) {
  if (a.vtx.size() != b.vtx.size() || a.idepths.size() != b.idepths.size()) return false;
  for (size_t i = 0; i < a.vtx.size(); ++i)
    if (std::memcmp(&a.vtx[i].x, &b.vtx[i].x, 4) || std::memcmp(&a.vtx[i].y, &b.vtx[i].y, 4)) return false;
  return a.idepths.empty() || !std::memcmp(a.idepths.data(), b.idepths.data(), 4 * a.idepths.size());
}

int main(int argc, char** argv) {
  if (argc < 2) return 10;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 11;
  std::fseek(f, 0, SEEK_END);
  const long size = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<char> buf(static_cast<size_t>(size));
  const bool read_ok = std::fread(buf.data(), 1, buf.size(), f) == buf.size();
  std::fclose(f);
  const size_t head = 20 + 20;
  if (!read_ok || buf.size() < head) return 11;
  int32_t hdr[5];
  float fl[5];
  std::memcpy(hdr, buf.data(), 20);
  std::memcpy(fl, buf.data() + 20, 20);
  const int W = hdr[0], H = hdr[1], frames = hdr[2];

  flame::Params plain;
  plain.hip_device = hdr[3];
  plain.nltgv2_iterations = hdr[4];
  flame::Params gated = plain;
  gated.do_letterbox = true;
  gated.min_height = fl[4];
  flame::Matrix3f K, Kinv;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K(r, c) = Kinv(r, c) = (r == c) ? 1.f : 0.f;
  K(0, 0) = fl[0]; K(1, 1) = fl[1]; K(0, 2) = fl[2]; K(1, 2) = fl[3];
  Kinv(0, 0) = 1.f / fl[0]; Kinv(1, 1) = 1.f / fl[1]; Kinv(0, 2) = -fl[2] / fl[0]; Kinv(1, 2) = -fl[3] / fl[1];

  // ---- a refused record, on a handle without a device ----
  bool all = true;
  {
    flame::Params bad = plain;
    bad.hip_device = -1;
    bad.min_height = 1.f;
    bad.max_height = 0.f;
    flame::GpuFrontEnd features(W, H, K, bad);
    flame::Image1b img(H, W);
    for (int y = 0; y < H; ++y) std::memset(img.ptr<uint8_t>(y), 0, W);
    const float q[4] = {0.f, 0.f, 0.f, 1.f}, t[3] = {0.f, 0.f, 0.f};
    flame::FrameInput in;
    in.img = &img;
    in.img_id = 1;
    in.pose = make_pose(q, t);
    in.is_poseframe = true;
    flame::FeatureSet out;
    const int e0 = features.lastError();
    const bool t0 = features.track(in, &out);
    const int e1 = features.lastError();
    const bool up0 = features.setUpAxis(0.f, 0.f, 0.f);  // (still min > max)
    const bool s1 = features.setGates(true, true, -1.f, 1.f);
    const int e2 = features.lastError();  // ARG again: the up axis is zero
    const bool up1 = features.setUpAxis(0.f, 1.f, 0.f);
    const int e3 = features.lastError();
    int64_t g = -1;
    flame_hip_frontend_info(features.handle(), "gates", &g);
    const bool t1 = features.track(in, &out);
    const int e4 = features.lastError();  // NODEVICE: the record is accepted, the handle has no device
    const bool s2 = features.setGates(false, false);
    int64_t g2 = -1;
    flame_hip_frontend_info(features.handle(), "gates", &g2);
    const bool refused = e0 == FLAME_HIP_ERR_ARG && !t0 && e1 == FLAME_HIP_ERR_ARG && !up0 && !s1 && e2 == FLAME_HIP_ERR_ARG && up1 && e3 == 0 &&
                         g == 3 && !t1 && e4 == FLAME_HIP_ERR_NODEVICE && s2 && g2 == 0;
    std::printf("refused=%d (%d %d %d %d %d gates %d %d)\n", refused ? 1 : 0, e0, e1, e2, e3, e4, static_cast<int>(g), static_cast<int>(g2));
    all = all && refused;
  }

  flame::Flame sensor_g(W, H, K, Kinv, gated), sensor_u(W, H, K, Kinv, plain), sensor_p(W, H, K, Kinv, plain);
  flame::GpuFrontEnd features_g(W, H, K, gated), features_u(W, H, K, plain);
  sensor_g.setFrontEnd(features_g.frontEnd());
  sensor_u.setFrontEnd(features_u.frontEnd());
  // P: the same handle parameters GpuFrontEnd uses, no gates anywhere
  flame_hip_frontend* raw = nullptr;
  flame_hip_frontend_params fp = features_u.frontendParams();
  {
    float Kr[9] = {fl[0], 0.f, fl[2], 0.f, fl[1], fl[3], 0.f, 0.f, 1.f};
    if (flame_hip_frontend_create(&raw, plain.hip_device, W, H, Kr, 4096, 16)) raw = nullptr;
    flame::FrontEnd fe;
    fe.track = [&raw, &fp](const flame::FrameInput& in, flame::FeatureSet* out) {
      if (!raw) return false;
      double T[12];
      flame::GpuFrontEnd::toRt(in.pose, T);
      const int32_t pitch = in.img->rows > 1 ? static_cast<int32_t>(in.img->ptr<uint8_t>(1) - in.img->ptr<uint8_t>(0)) : in.img->cols;
      int32_t n = 0;
      if (flame_hip_frontend_track(raw, &fp, in.img->ptr<uint8_t>(0), pitch, in.img_id, T, in.is_poseframe ? 1 : 0, &n)) return false;
      out->vtx.resize(static_cast<size_t>(n));
      out->idepth_mu.resize(static_cast<size_t>(n));
      out->idepth_var.resize(static_cast<size_t>(n));
      out->prediction.clear();
      if (flame_hip_frontend_features(raw, n, n ? reinterpret_cast<float*>(out->vtx.data()) : nullptr, out->idepth_mu.data(),
                                      out->idepth_var.data(), nullptr, nullptr))
        return false;
      return n >= 3;
    };
    fe.updatePoseFramePoses = [&raw](const std::vector<uint32_t>& ids, const std::vector<flame::SE3f>& poses) {
      if (!raw || ids.size() != poses.size()) return;
      std::vector<double> T(12 * ids.size());
      for (size_t i = 0; i < ids.size(); ++i) flame::GpuFrontEnd::toRt(poses[i], &T[12 * i]);
      flame_hip_frontend_set_poses(raw, static_cast<int32_t>(ids.size()), ids.data(), T.data());
    };
    fe.prunePoseFrames = [&raw](const std::vector<uint32_t>& ids) {
      if (raw) flame_hip_frontend_prune(raw, static_cast<int32_t>(ids.size()), ids.data());
    };
    sensor_p.setFrontEnd(fe);
  }
  int64_t gg = -1, gu = -1;
  if (features_g.handle()) flame_hip_frontend_info(features_g.handle(), "gates", &gg);
  if (features_u.handle()) flame_hip_frontend_info(features_u.handle(), "gates", &gu);
  std::printf("gates_g=%d gates_u=%d\n", static_cast<int>(gg), static_cast<int>(gu));

  const int y_lo = H / 3, y_hi = H - H / 3;
  const size_t rec = 8 + 28 + static_cast<size_t>(W) * H;
  bool ok_g = false, ok_u = false, ok_p = false;
  flame::Image1b img(H, W);
  for (int k = 0; k < frames; ++k) {
    const char* p = buf.data() + head + rec * k;
    if (p + rec > buf.data() + buf.size()) return 11;
    int32_t ih[2];
    float qt[7];
    std::memcpy(ih, p, 8);
    std::memcpy(qt, p + 8, 28);
    for (int y = 0; y < H; ++y) std::memcpy(img.ptr<uint8_t>(y), p + 36 + static_cast<size_t>(y) * W, W);
    const flame::SE3f pose = make_pose(qt, qt + 4);
    const uint32_t id = static_cast<uint32_t>(ih[0]);
    ok_g = sensor_g.update(0.1 * k, id, pose, img, ih[1] != 0);
    ok_u = sensor_u.update(0.1 * k, id, pose, img, ih[1] != 0);
    ok_p = sensor_p.update(0.1 * k, id, pose, img, ih[1] != 0);
    const Mesh mg = mesh_of(sensor_g), mu = mesh_of(sensor_u), mp = mesh_of(sensor_p);
    bool in_band = true;
    for (size_t i = 0; i < mg.vtx.size(); ++i) in_band = in_band && mg.vtx[i].y >= static_cast<float>(y_lo) && mg.vtx[i].y <= static_cast<float>(y_hi - 1);
    bool u_outside = false;
    for (size_t i = 0; i < mu.vtx.size(); ++i) u_outside = u_outside || mu.vtx[i].y < static_cast<float>(y_lo) || mu.vtx[i].y > static_cast<float>(y_hi - 1);
    const bool mesh_same = ok_u == ok_p && same(mu, mp);
    all = all && in_band && mesh_same;
    const int err = features_g.lastError() ? features_g.lastError() : static_cast<int>(sensor_g.stats().stats("hip_error"));
    std::printf("frame=%d update_g=%d update_u=%d update_p=%d hip_error=%d vtx_g=%d vtx_u=%d in_band=%d u_outside=%d mesh_same=%d held=%d "
                "refused=%d held_u=%d\n",
                k, ok_g ? 1 : 0, ok_u ? 1 : 0, ok_p ? 1 : 0, ok_g ? 0 : err, static_cast<int>(mg.vtx.size()), static_cast<int>(mu.vtx.size()),
                in_band ? 1 : 0, u_outside ? 1 : 0, mesh_same ? 1 : 0, static_cast<int>(sensor_g.stats().stats("num_held_height")),
                static_cast<int>(sensor_g.stats().stats("num_refused_letterbox")), static_cast<int>(sensor_u.stats().stats("num_held_height")));
  }
  flame_hip_frontend_destroy(raw);
  if (!all) return 4;
  return (ok_g && ok_u && ok_p) ? 0 : 3;
}
