// tests/cpp/fe_gi_facade.cc -- the gain-invariant matching cost behind flame::GpuFrontEnd (Params::gain_invariant_matching,
// setGainInvariant): six Flame + front-end pairs over one sequence of grey frames and its gained copy (every frame that is no pose
// frame 2 v + b, every pose frame v + |b|) --
//   G0 / G1: Params::gain_invariant_matching on, the plain sequence / the gained copy;
//   Z0 / Z1: Params::zero_mean_matching alone, the plain sequence / the gained copy;
//   S0:      the defaults (SSD) on the plain sequence;
//   P:       the defaults on the plain sequence, the FrontEnd's `track` written here on a handle of its own with
//            flame_hip_frontend_track / _features alone -- a pair built without any call of a matching cost.
// After every update(): G0's mesh equals G1's byte for byte and S0's equals P's; over the whole sequence Z0's and Z1's differ.
// Before the frames, on a handle without a device (hip_device = -1): the constructor sets the switch Params asks for and leaves
// "cost_mode" alone, setGainInvariant() changes it, track() fails with NODEVICE; on a handle that could not be made
// setGainInvariant() returns false and lastError() keeps the reason.  Compiles with the fallback types and with the cv:: / Eigen:: /
// Sophus:: stand-ins.
// Usage: fe_gi_facade in.bin.  in.bin: int32 {W, H, frames, device, iterations, win_size}, float32 {fx, fy, cx, cy}, then 2 x frames
// records (the plain sequence, then the gained copy) of int32 {img_id, is_poseframe}, float32 {qx, qy, qz, qw, tx, ty, tz}, W x H
// grey bytes.  One line per frame; exit code 0 = every check held and the last updates succeeded, 3 = a last update failed, 4 = a
// check failed.
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
static int64_t info(const flame::GpuFrontEnd& fe, const char* key) {
  int64_t v = -1;
  if (fe.handle()) flame_hip_frontend_info(fe.handle(), key, &v);
  return v;
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
  plain.zparams.win_size = hdr[5];
  flame::Params zm = plain;
  zm.zero_mean_matching = true;
  flame::Params gi = plain;
  gi.gain_invariant_matching = true;
  flame::Matrix3f K, Kinv;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K(r, c) = Kinv(r, c) = (r == c) ? 1.f : 0.f;
  K(0, 0) = fl[0]; K(1, 1) = fl[1]; K(0, 2) = fl[2]; K(1, 2) = fl[3];
  Kinv(0, 0) = 1.f / fl[0]; Kinv(1, 1) = 1.f / fl[1]; Kinv(0, 2) = -fl[2] / fl[0]; Kinv(1, 2) = -fl[3] / fl[1];

  // ---- the switch, on a handle without a device and on no handle at all ----
  bool all = true;
  {
    flame::Params nodev = gi;
    nodev.hip_device = -1;
    flame::GpuFrontEnd features(W, H, K, nodev);
    const int e0 = features.lastError();
    const int64_t g0 = info(features, "gain_invariant"), m0 = info(features, "cost_mode");
    const bool b0 = features.gainInvariant();
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
    const bool s0 = features.setGainInvariant(false);
    const int64_t g1 = info(features, "gain_invariant");
    const bool s1 = features.setGainInvariant(true);
    const int64_t g2 = info(features, "gain_invariant");
    nodev.gain_invariant_matching = false;
    nodev.zero_mean_matching = true;
    flame::GpuFrontEnd untouched(W, H, K, nodev);
    const int64_t g3 = info(untouched, "gain_invariant"), m3 = info(untouched, "cost_mode");
    flame::GpuFrontEnd none(4, 4, K, gi);  // (an image the library refuses: no handle)
    const int e2 = none.lastError();
    const bool s2 = none.setGainInvariant(true);
    const int e3 = none.lastError();
    const bool t1 = none.track(in, &out);
    const bool surface = e0 == 0 && g0 == 1 && m0 == FLAME_HIP_FE_COST_SSD && b0 && !t0 && e1 == FLAME_HIP_ERR_NODEVICE && s0 && g1 == 0 && s1 &&
                         g2 == 1 && g3 == 0 && m3 == FLAME_HIP_FE_COST_ZSSD && !untouched.gainInvariant() && e2 == FLAME_HIP_ERR_ARG && !s2 &&
                         e3 == FLAME_HIP_ERR_ARG && !t1;
    std::printf("surface=%d (%d %d %d %d switch %d %d %d %d modes %d %d)\n", surface ? 1 : 0, e0, e1, e2, e3, static_cast<int>(g0),
                static_cast<int>(g1), static_cast<int>(g2), static_cast<int>(g3), static_cast<int>(m0), static_cast<int>(m3));
    all = all && surface;
  }

  flame::Flame sensor_g0(W, H, K, Kinv, gi), sensor_g1(W, H, K, Kinv, gi), sensor_z0(W, H, K, Kinv, zm), sensor_z1(W, H, K, Kinv, zm),
      sensor_s0(W, H, K, Kinv, plain), sensor_p(W, H, K, Kinv, plain);
  flame::GpuFrontEnd features_g0(W, H, K, gi), features_g1(W, H, K, gi), features_z0(W, H, K, zm), features_z1(W, H, K, zm),
      features_s0(W, H, K, plain);
  sensor_g0.setFrontEnd(features_g0.frontEnd());
  sensor_g1.setFrontEnd(features_g1.frontEnd());
  sensor_z0.setFrontEnd(features_z0.frontEnd());
  sensor_z1.setFrontEnd(features_z1.frontEnd());
  sensor_s0.setFrontEnd(features_s0.frontEnd());
  // P: the same handle parameters GpuFrontEnd uses, no matching-cost call anywhere
  flame_hip_frontend* raw = nullptr;
  flame_hip_frontend_params fp = features_s0.frontendParams();
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
  std::printf("gi_g=%d gi_z=%d gi_s=%d cost_g=%d cost_z=%d\n", static_cast<int>(info(features_g0, "gain_invariant")),
              static_cast<int>(info(features_z0, "gain_invariant")), static_cast<int>(info(features_s0, "gain_invariant")),
              static_cast<int>(info(features_g0, "cost_mode")), static_cast<int>(info(features_z0, "cost_mode")));

  const size_t rec = 8 + 28 + static_cast<size_t>(W) * H;
  if (buf.size() < head + rec * 2 * static_cast<size_t>(frames)) return 11;
  bool ok_g0 = false, ok_g1 = false, ok_z0 = false, ok_z1 = false, ok_s0 = false, ok_p = false, zssd_moved = false;
  flame::Image1b img(H, W), img_off(H, W);
  for (int k = 0; k < frames; ++k) {
    const char* p = buf.data() + head + rec * k;
    const char* po = buf.data() + head + rec * (frames + k);
    int32_t ih[2];
    float qt[7];
    std::memcpy(ih, p, 8);
    std::memcpy(qt, p + 8, 28);
    bool differs = false;
    for (int y = 0; y < H; ++y) {
      std::memcpy(img.ptr<uint8_t>(y), p + 36 + static_cast<size_t>(y) * W, W);
      std::memcpy(img_off.ptr<uint8_t>(y), po + 36 + static_cast<size_t>(y) * W, W);
      differs = differs || std::memcmp(img.ptr<uint8_t>(y), img_off.ptr<uint8_t>(y), W) != 0;
    }
    const flame::SE3f pose = make_pose(qt, qt + 4);
    const uint32_t id = static_cast<uint32_t>(ih[0]);
    ok_g0 = sensor_g0.update(0.1 * k, id, pose, img, ih[1] != 0);
    ok_g1 = sensor_g1.update(0.1 * k, id, pose, img_off, ih[1] != 0);
    ok_z0 = sensor_z0.update(0.1 * k, id, pose, img, ih[1] != 0);
    ok_z1 = sensor_z1.update(0.1 * k, id, pose, img_off, ih[1] != 0);
    ok_s0 = sensor_s0.update(0.1 * k, id, pose, img, ih[1] != 0);
    ok_p = sensor_p.update(0.1 * k, id, pose, img, ih[1] != 0);
    const Mesh g0 = mesh_of(sensor_g0), g1 = mesh_of(sensor_g1), z0 = mesh_of(sensor_z0), z1 = mesh_of(sensor_z1), s0 = mesh_of(sensor_s0),
               mp = mesh_of(sensor_p);
    const bool gi_same = ok_g0 == ok_g1 && same(g0, g1);
    const bool zssd_same = ok_z0 == ok_z1 && same(z0, z1);
    const bool plain_same = ok_s0 == ok_p && same(s0, mp);
    zssd_moved = zssd_moved || !zssd_same;
    all = all && gi_same && plain_same && differs;
    const int err = features_g0.lastError() ? features_g0.lastError() : static_cast<int>(sensor_g0.stats().stats("hip_error"));
    std::printf("frame=%d update_g0=%d update_g1=%d update_z0=%d update_z1=%d update_s0=%d update_p=%d hip_error=%d vtx_g0=%d vtx_z0=%d vtx_s0=%d "
                "images_differ=%d gi_same=%d zssd_same=%d plain_same=%d\n",
                k, ok_g0 ? 1 : 0, ok_g1 ? 1 : 0, ok_z0 ? 1 : 0, ok_z1 ? 1 : 0, ok_s0 ? 1 : 0, ok_p ? 1 : 0, ok_g0 ? 0 : err,
                static_cast<int>(g0.vtx.size()), static_cast<int>(z0.vtx.size()), static_cast<int>(s0.vtx.size()), differs ? 1 : 0,
                gi_same ? 1 : 0, zssd_same ? 1 : 0, plain_same ? 1 : 0);
  }
  flame_hip_frontend_destroy(raw);
  std::printf("zssd_moved=%d\n", zssd_moved ? 1 : 0);
  if (!all) return 4;
  if (!(ok_g0 && ok_g1 && ok_s0 && ok_p)) return 3;
  return zssd_moved ? 0 : 4;
}
