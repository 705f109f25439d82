// tests/cpp/ingest_facade.cc -- two flame::Flame + flame::GpuFrontEnd pairs over one sequence of RAW (distorted) grey images:
// pair A has GpuFrontEnd::setCamera and takes the raw frames (the library's ingest stage rectifies them on the GPU), pair B
// takes the frames rectified on the host by include/flame_ros/image_io.h undistort<uint8_t>.  Everything Flame hands out must
// be identical: vertices, idepths, triangles, validity, and with Params::photo_error the photo keys (A's evaluate stage reads
// the rectified image through FrontEnd::rectified).  Compiles with the fallback types and with the cv:: / Eigen:: / Sophus::
// stand-ins.
// Usage: ingest_facade in.bin.  in.bin: int32 {W, H, frames, device, iterations, photo_error}, float32 {fx, fy, cx, cy,
// idepth_var_max_graph, k1, k2, p1, p2, k3}, then per frame int32 {img_id, is_poseframe}, float32 {qx, qy, qz, qw, tx, ty, tz},
// W x H raw grey bytes.  One line per frame; exit code 0 = every frame identical and the last update succeeded, 3 = the last
// update failed, 4 = a difference.
#include <cstdio>
#include <cstring>
#include <vector>

#include "flame/flame.h"
#include "flame/gpu_frontend.h"
#include "flame_ros/image_io.h"

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
  std::vector<flame::Triangle> tris;
  std::vector<bool> valid;
  double photo[3];
};

static void take(const flame::Flame& s, Mesh* m) {
  s.getInverseDepthMesh(&m->vtx, &m->idepths, nullptr, &m->tris, &m->valid, nullptr);
  m->photo[0] = s.stats().stats("total_photo_error");
  m->photo[1] = s.stats().stats("avg_photo_error");
  m->photo[2] = s.stats().stats("photo_pixels");
}

static bool same_mesh(const Mesh& a, const Mesh& b) {
  if (a.vtx.size() != b.vtx.size() || a.idepths.size() != b.idepths.size() || a.tris.size() != b.tris.size() || a.valid != b.valid) return false;
  for (size_t i = 0; i < a.vtx.size(); ++i)
    if (std::memcmp(&a.vtx[i].x, &b.vtx[i].x, 4) || std::memcmp(&a.vtx[i].y, &b.vtx[i].y, 4)) return false;
  if (!a.idepths.empty() && std::memcmp(a.idepths.data(), b.idepths.data(), 4 * a.idepths.size())) return false;
  for (size_t i = 0; i < a.tris.size(); ++i)
    for (int k = 0; k < 3; ++k)
      if (a.tris[i][k] != b.tris[i][k]) return false;
  return true;
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
  const size_t head = 24 + 40;
  if (!read_ok || buf.size() < head) return 11;
  int32_t hdr[6];
  float fl[10];
  std::memcpy(hdr, buf.data(), 24);
  std::memcpy(fl, buf.data() + 24, 40);
  const int W = hdr[0], H = hdr[1], frames = hdr[2];

  flame::Params params;
  params.hip_device = hdr[3];
  params.nltgv2_iterations = hdr[4];
  params.photo_error = hdr[5] != 0;
  params.idepth_var_max_graph = fl[4];
  flame::Matrix3f K, Kinv;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K(r, c) = Kinv(r, c) = (r == c) ? 1.f : 0.f;
  K(0, 0) = fl[0]; K(1, 1) = fl[1]; K(0, 2) = fl[2]; K(1, 2) = fl[3];
  Kinv(0, 0) = 1.f / fl[0]; Kinv(1, 1) = 1.f / fl[1]; Kinv(0, 2) = -fl[2] / fl[0]; Kinv(1, 2) = -fl[3] / fl[1];
  flame_ros::images::PlumbBob cam;
  cam.fx = fl[0]; cam.fy = fl[1]; cam.cx = fl[2]; cam.cy = fl[3];
  cam.k1 = fl[5]; cam.k2 = fl[6]; cam.p1 = fl[7]; cam.p2 = fl[8]; cam.k3 = fl[9];

  flame::Flame sensor_a(W, H, K, Kinv, params), sensor_b(W, H, K, Kinv, params);
  flame::GpuFrontEnd features_a(W, H, K, params), features_b(W, H, K, params);
  const bool cam_ok = features_a.setCamera(W, H, 1, fl + 5);
  sensor_a.setFrontEnd(features_a.frontEnd());
  sensor_b.setFrontEnd(features_b.frontEnd());
  std::printf("camera=%d rectified_bound=%d/%d\n", cam_ok ? 1 : 0, features_a.frontEnd().rectified ? 1 : 0, features_b.frontEnd().rectified ? 1 : 0);

  const size_t rec = 8 + 28 + static_cast<size_t>(W) * H;
  bool ok_a = false, all_same = true;
  flame::Image1b raw(H, W), rect(H, W);
  std::vector<uint8_t> raw_dense(static_cast<size_t>(W) * H), rect_dense(raw_dense.size());
  for (int k = 0; k < frames; ++k) {
    const char* p = buf.data() + head + rec * k;
    if (p + rec > buf.data() + buf.size()) return 11;
    int32_t ih[2];
    float qt[7];
    std::memcpy(ih, p, 8);
    std::memcpy(qt, p + 8, 28);
    std::memcpy(raw_dense.data(), p + 36, raw_dense.size());
    flame_ros::images::undistort<uint8_t>(raw_dense.data(), W, H, 1, cam, rect_dense.data());
    for (int y = 0; y < H; ++y) {
      std::memcpy(raw.ptr<uint8_t>(y), raw_dense.data() + static_cast<size_t>(y) * W, W);
      std::memcpy(rect.ptr<uint8_t>(y), rect_dense.data() + static_cast<size_t>(y) * W, W);
    }
    const flame::SE3f pose = make_pose(qt, qt + 4);
    ok_a = sensor_a.update(0.1 * k, static_cast<uint32_t>(ih[0]), pose, raw, ih[1] != 0);
    const bool ok_b = sensor_b.update(0.1 * k, static_cast<uint32_t>(ih[0]), pose, rect, ih[1] != 0);
    Mesh a, b;
    take(sensor_a, &a);
    take(sensor_b, &b);
    const bool same = ok_a == ok_b && same_mesh(a, b);
    const bool photo_same = !std::memcmp(a.photo, b.photo, sizeof(a.photo));
    all_same = all_same && same && photo_same;
    const int err = features_a.lastError() ? features_a.lastError() : static_cast<int>(sensor_a.stats().stats("hip_error"));
    int valid = 0;
    for (size_t i = 0; i < a.valid.size(); ++i) valid += a.valid[i] ? 1 : 0;
    std::printf("frame=%d update=%d/%d hip_error=%d same=%d photo_same=%d vtx=%d tris=%d valid=%d photo_total=%.6f photo_pixels=%d\n", k,
                ok_a ? 1 : 0, ok_b ? 1 : 0, ok_a ? 0 : err, same ? 1 : 0, photo_same ? 1 : 0, static_cast<int>(a.vtx.size()),
                static_cast<int>(a.tris.size()), valid, a.photo[0], static_cast<int>(a.photo[2]));
  }
  if (!all_same) return 4;
  return ok_a ? 0 : 3;
}
