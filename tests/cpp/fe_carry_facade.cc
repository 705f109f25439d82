// tests/cpp/fe_carry_facade.cc -- the hand-over of an evicted pose frame's features behind flame::GpuFrontEnd
// (Params::carry_features, setCarry): three Flame + front-end pairs with a pose-frame ring of `ring` slots over one sequence of grey
// frames --
//   C: Params::carry_features = true;
//   D: the defaults (switch off);
//   P: the FrontEnd's `track` written here on a handle of its own with flame_hip_frontend_set_carry(1) and flame_hip_frontend_track /
//      _features alone -- the library call itself.
// After every update(): C's mesh equals P's byte for byte (the frame's features are the library call's), D's stats hold neither
// num_carried nor num_carry_lost, C's do and they equal the info keys "carried" / "carry_lost".  `graph` is the number of the frame's
// features that pass Flame's variance gate (emitted - num_fail_max_var): the vertices of the frame's graph.  C's mesh of every frame
// goes to out.bin, D's behind it.
// Before the frames, on a handle without a device (hip_device = -1): the constructor sets the switch Params asks for, setCarry()
// changes it, track() fails with NODEVICE; on a handle that could not be made setCarry() returns false and lastError() keeps the
// reason.  Compiles with the fallback types and with the cv:: / Eigen:: / Sophus:: stand-ins.
// Usage: fe_carry_facade in.bin out.bin.  in.bin: int32 {W, H, frames, device, iterations, ring}, float32 {fx, fy, cx, cy},
// then `frames` records of int32 {img_id, is_poseframe}, float32 {qx, qy, qz, qw, tx, ty, tz}, W x H grey bytes.  out.bin: per frame
// and per pair (C, then D) int32 n, then n x float32 {x, y, idepth}.  One line per frame; exit code 0 = every check held and the last
// updates succeeded, 3 = a last update failed, 4 = a check failed.
#include <cmath>
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
static void write_mesh(FILE* f, const Mesh& m) {
  const int32_t n = static_cast<int32_t>(m.vtx.size() == m.idepths.size() ? m.vtx.size() : 0);
  std::fwrite(&n, 4, 1, f);
  for (int32_t i = 0; i < n; ++i) {
    const float r[3] = {m.vtx[i].x, m.vtx[i].y, m.idepths[i]};
    std::fwrite(r, 4, 3, f);
  }
}
static int64_t info(const flame::GpuFrontEnd& fe, const char* key) {
  int64_t v = -1;
  if (fe.handle()) flame_hip_frontend_info(fe.handle(), key, &v);
  return v;
}
static int stat_or_minus1(const flame::Flame& sensor, const char* key) {
  const flame::utils::StatsTracker& s = sensor.stats();
  return s.stats().count(key) ? static_cast<int>(s.stats(key)) : -1;
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
  const size_t head = 24 + 16;
  if (!read_ok || buf.size() < head) return 11;
  int32_t hdr[6];
  float fl[4];
  std::memcpy(hdr, buf.data(), 24);
  std::memcpy(fl, buf.data() + 24, 16);
  const int W = hdr[0], H = hdr[1], frames = hdr[2];

  flame::Params plain;
  plain.hip_device = hdr[3];
  plain.nltgv2_iterations = hdr[4];
  const int ring = hdr[5];
  flame::Params carrying = plain;
  carrying.carry_features = true;
  flame::Matrix3f K, Kinv;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K(r, c) = Kinv(r, c) = (r == c) ? 1.f : 0.f;
  K(0, 0) = fl[0]; K(1, 1) = fl[1]; K(0, 2) = fl[2]; K(1, 2) = fl[3];
  Kinv(0, 0) = 1.f / fl[0]; Kinv(1, 1) = 1.f / fl[1]; Kinv(0, 2) = -fl[2] / fl[0]; Kinv(1, 2) = -fl[3] / fl[1];

  // ---- the switch, on a handle without a device and on no handle at all ----
  bool all = true;
  {
    flame::Params nodev = carrying;
    nodev.hip_device = -1;
    flame::GpuFrontEnd features(W, H, K, nodev, 256, ring);
    const int e0 = features.lastError();
    const int64_t g0 = info(features, "carry");
    const bool v0 = features.carry();
    flame::Image1b img(H, W);
    for (int y = 0; y < H; ++y) std::memset(img.ptr<uint8_t>(y), 0, W);
    const float q[4] = {0.f, 0.f, 0.f, 1.f}, t[3] = {0.f, 0.f, 0.f};
    flame::FrameInput in;
    in.img = &img;
    in.img_id = 1;
    in.pose = make_pose(q, t);
    in.is_poseframe = true;
    flame::FeatureSet out;
    const bool t0 = features.track(in, &out);
    const int e1 = features.lastError();  // NODEVICE: the switch is accepted, the handle has no device
    const bool s0 = features.setCarry(false);
    const int64_t g1 = info(features, "carry");
    const bool v1 = features.carry();
    const bool s1 = features.setCarry(true);
    const int64_t g2 = info(features, "carry");
    const bool t1 = features.track(in, &out);
    const int e2 = features.lastError();  // NODEVICE again
    nodev.carry_features = false;
    flame::GpuFrontEnd untouched(W, H, K, nodev, 256, ring);
    const int64_t g3 = info(untouched, "carry");
    flame::GpuFrontEnd none(4, 4, K, carrying);  // (an image the library refuses: no handle)
    const int e3 = none.lastError();
    const bool s2 = none.setCarry(true);
    const int e4 = none.lastError();
    const bool surface = e0 == 0 && g0 == 1 && v0 && !t0 && e1 == FLAME_HIP_ERR_NODEVICE && s0 && g1 == 0 && !v1 && s1 && g2 == 1 && features.carry() &&
                         !t1 && e2 == FLAME_HIP_ERR_NODEVICE && g3 == 0 && !untouched.carry() && e3 == FLAME_HIP_ERR_ARG && !s2 && !none.carry() &&
                         e4 == FLAME_HIP_ERR_ARG;
    std::printf("surface=%d (%d %d %d %d %d carry %d %d %d %d)\n", surface ? 1 : 0, e0, e1, e2, e3, e4, static_cast<int>(g0), static_cast<int>(g1),
                static_cast<int>(g2), static_cast<int>(g3));
    all = all && surface;
  }

  flame::Flame sensor_c(W, H, K, Kinv, carrying), sensor_d(W, H, K, Kinv, plain), sensor_p(W, H, K, Kinv, plain);
  flame::GpuFrontEnd features_c(W, H, K, carrying, 256, ring), features_d(W, H, K, plain, 256, ring);
  sensor_c.setFrontEnd(features_c.frontEnd());
  sensor_d.setFrontEnd(features_d.frontEnd());
  // P: the same handle parameters GpuFrontEnd uses, the switch set by the library call
  flame_hip_frontend* raw = nullptr;
  flame_hip_frontend_params fp = features_d.frontendParams();
  {
    float Kr[9] = {fl[0], 0.f, fl[2], 0.f, fl[1], fl[3], 0.f, 0.f, 1.f};
    if (flame_hip_frontend_create(&raw, plain.hip_device, W, H, Kr, 256, ring)) raw = nullptr;
    if (raw && flame_hip_frontend_set_carry(raw, 1)) all = false;
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
  std::printf("carry_c=%d carry_d=%d\n", static_cast<int>(info(features_c, "carry")), static_cast<int>(info(features_d, "carry")));

  const size_t rec = 8 + 28 + static_cast<size_t>(W) * H;
  if (buf.size() < head + rec * static_cast<size_t>(frames)) return 11;
  FILE* fo = std::fopen(argv[2], "wb");
  if (!fo) return 12;
  bool ok_c = false, ok_d = false, ok_p = false;
  flame::Image1b img(H, W);
  for (int k = 0; k < frames; ++k) {
    const char* p = buf.data() + head + rec * k;
    int32_t ih[2];
    float qt[7];
    std::memcpy(ih, p, 8);
    std::memcpy(qt, p + 8, 28);
    for (int y = 0; y < H; ++y) std::memcpy(img.ptr<uint8_t>(y), p + 36 + static_cast<size_t>(y) * W, W);
    const flame::SE3f pose = make_pose(qt, qt + 4);
    const uint32_t id = static_cast<uint32_t>(ih[0]);
    ok_c = sensor_c.update(0.1 * k, id, pose, img, ih[1] != 0);
    ok_d = sensor_d.update(0.1 * k, id, pose, img, ih[1] != 0);
    ok_p = sensor_p.update(0.1 * k, id, pose, img, ih[1] != 0);
    const Mesh mc = mesh_of(sensor_c), md = mesh_of(sensor_d), mp = mesh_of(sensor_p);
    write_mesh(fo, mc);
    write_mesh(fo, md);
    const bool abi_same = ok_c == ok_p && same(mc, mp);
    const int carried_c = stat_or_minus1(sensor_c, "num_carried"), lost_c = stat_or_minus1(sensor_c, "num_carry_lost");
    const int carried_d = stat_or_minus1(sensor_d, "num_carried"), lost_d = stat_or_minus1(sensor_d, "num_carry_lost");
    const int graph_c = static_cast<int>(info(features_c, "emitted")) - stat_or_minus1(sensor_c, "num_fail_max_var");
    const int graph_d = static_cast<int>(info(features_d, "emitted")) - stat_or_minus1(sensor_d, "num_fail_max_var");
    all = all && abi_same && carried_d == -1 && lost_d == -1;
    const int err = features_c.lastError() ? features_c.lastError() : static_cast<int>(sensor_c.stats().stats("hip_error"));
    std::printf("frame=%d update_c=%d update_d=%d update_p=%d hip_error=%d vtx_c=%d vtx_d=%d graph_c=%d graph_d=%d carried_c=%d lost_c=%d "
                "carried_d=%d lost_d=%d info_carried=%d info_lost=%d abi_same=%d\n",
                k, ok_c ? 1 : 0, ok_d ? 1 : 0, ok_p ? 1 : 0, ok_c ? 0 : err, static_cast<int>(mc.vtx.size()), static_cast<int>(md.vtx.size()),
                graph_c, graph_d, carried_c, lost_c, carried_d, lost_d, static_cast<int>(info(features_c, "carried")),
                static_cast<int>(info(features_c, "carry_lost")), abi_same ? 1 : 0);
  }
  std::fclose(fo);
  flame_hip_frontend_destroy(raw);
  if (!all) return 4;
  return (ok_c && ok_d && ok_p) ? 0 : 3;
}
