// tests/cpp/fe_debug_facade.cc -- flame::Flame::getDebugImageDetections() / getDebugImageMatches() behind a flame::GpuFrontEnd
// (FrontEnd::debugImage): four Flame + GpuFrontEnd pairs over one sequence of grey frames --
//   A: both flags on, the callback wrapped in a counter;   B: as A with Params::debug_flip_images;
//   C: both flags off;                                     D: both flags on, the callback taken out of the FrontEnd.
// After every update(): A's pictures must equal flame_hip_frontend_debug_image called directly on A's handle (also on a frame
// whose update failed at the variance gate), a second getter call must return the same object without another render, B's must
// be the 180 degree rotation of the direct pictures of B's handle, C's and D's black.  Compiles with the fallback types and with
// the cv:: / Eigen:: / Sophus:: stand-ins.
// Usage: fe_debug_facade in.bin.  in.bin: int32 {W, H, frames, device, iterations}, float32 {fx, fy, cx, cy}, then per frame
// int32 {img_id, is_poseframe}, float32 {qx, qy, qz, qw, tx, ty, tz}, W x H grey bytes.  One line per frame; exit code 0 = every
// check held and the last update succeeded, 3 = the last update failed, 4 = a check failed.
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

// dense BGR bytes of a picture
static std::vector<uint8_t> bytes(const flame::Image3b& img) {
  std::vector<uint8_t> b(3 * static_cast<size_t>(img.rows) * img.cols);
  for (int y = 0; y < img.rows; ++y)
    for (int x = 0; x < img.cols; ++x)
      for (int c = 0; c < 3; ++c) b[3 * (static_cast<size_t>(y) * img.cols + x) + c] = img(y, x)[c];
  return b;
}
static bool direct(const flame::GpuFrontEnd& fe, int kind, int W, int H, std::vector<uint8_t>* out) {
  out->assign(3 * static_cast<size_t>(W) * H, 0);
  return fe.handle() && flame_hip_frontend_debug_image(fe.handle(), kind, out->data(), 3 * W) == 0;
}
static std::vector<uint8_t> rotated(const std::vector<uint8_t>& b) {
  std::vector<uint8_t> r(b.size());
  const size_t n = b.size() / 3;
  for (size_t i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) r[3 * (n - 1 - i) + c] = b[3 * i + c];
  return r;
}
static bool black(const std::vector<uint8_t>& b) {
  for (size_t i = 0; i < b.size(); ++i)
    if (b[i]) return false;
  return true;
}
static int coloured(const std::vector<uint8_t>& b) {
  int n = 0;
  for (size_t i = 0; i + 2 < b.size(); i += 3) n += (b[i] != b[i + 1] || b[i + 1] != b[i + 2]) ? 1 : 0;
  return n;
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
  const size_t head = 20 + 16;
  if (!read_ok || buf.size() < head) return 11;
  int32_t hdr[5];
  float fl[4];
  std::memcpy(hdr, buf.data(), 20);
  std::memcpy(fl, buf.data() + 20, 16);
  const int W = hdr[0], H = hdr[1], frames = hdr[2];

  flame::Params on;
  on.hip_device = hdr[3];
  on.nltgv2_iterations = hdr[4];
  on.debug_draw_detections = true;
  on.debug_draw_matches = true;
  flame::Params flip = on, off = on;
  flip.debug_flip_images = true;
  off.debug_draw_detections = false;
  off.debug_draw_matches = false;
  flame::Matrix3f K, Kinv;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) K(r, c) = Kinv(r, c) = (r == c) ? 1.f : 0.f;
  K(0, 0) = fl[0]; K(1, 1) = fl[1]; K(0, 2) = fl[2]; K(1, 2) = fl[3];
  Kinv(0, 0) = 1.f / fl[0]; Kinv(1, 1) = 1.f / fl[1]; Kinv(0, 2) = -fl[2] / fl[0]; Kinv(1, 2) = -fl[3] / fl[1];

  flame::Flame sensor_a(W, H, K, Kinv, on), sensor_b(W, H, K, Kinv, flip), sensor_c(W, H, K, Kinv, off), sensor_d(W, H, K, Kinv, on);
  flame::GpuFrontEnd features_a(W, H, K, on), features_b(W, H, K, flip), features_c(W, H, K, off), features_d(W, H, K, on);
  int renders = 0;
  {
    flame::FrontEnd fe = features_a.frontEnd();
    const std::function<bool(int, flame::Image3b*)> inner = fe.debugImage;
    fe.debugImage = [&renders, inner](int kind, flame::Image3b* out) { ++renders; return inner(kind, out); };
    sensor_a.setFrontEnd(fe);
    sensor_b.setFrontEnd(features_b.frontEnd());
    sensor_c.setFrontEnd(features_c.frontEnd());
    flame::FrontEnd fd = features_d.frontEnd();
    std::printf("callback_bound=%d\n", fd.debugImage ? 1 : 0);
    fd.debugImage = nullptr;
    sensor_d.setFrontEnd(fd);
  }
  // before the first update: black, and nothing is rendered
  bool all = black(bytes(sensor_a.getDebugImageMatches())) && black(bytes(sensor_a.getDebugImageDetections())) && renders == 0;
  std::printf("before=%d\n", all ? 1 : 0);

  const size_t rec = 8 + 28 + static_cast<size_t>(W) * H;
  bool ok_a = false;
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
    ok_a = sensor_a.update(0.1 * k, id, pose, img, ih[1] != 0);
    sensor_b.update(0.1 * k, id, pose, img, ih[1] != 0);
    sensor_c.update(0.1 * k, id, pose, img, ih[1] != 0);
    sensor_d.update(0.1 * k, id, pose, img, ih[1] != 0);

    std::vector<uint8_t> dm, dd, bm, bd;
    const bool have = direct(features_a, FLAME_HIP_FE_IMG_MATCHES, W, H, &dm) && direct(features_a, FLAME_HIP_FE_IMG_DETECTIONS, W, H, &dd) &&
                      direct(features_b, FLAME_HIP_FE_IMG_MATCHES, W, H, &bm) && direct(features_b, FLAME_HIP_FE_IMG_DETECTIONS, W, H, &bd);
    const int before = renders;
    const flame::Image3b& m1 = sensor_a.getDebugImageMatches();
    const flame::Image3b& d1 = sensor_a.getDebugImageDetections();
    const int after_first = renders;
    const flame::Image3b& m2 = sensor_a.getDebugImageMatches();
    const flame::Image3b& d2 = sensor_a.getDebugImageDetections();
    const bool cached = &m1 == &m2 && &d1 == &d2 && renders == after_first && bytes(m2) == bytes(m1) && bytes(d2) == bytes(d1);
    const bool same_m = bytes(m1) == dm, same_d = bytes(d1) == dd;
    const bool flip_same = bytes(sensor_b.getDebugImageMatches()) == rotated(bm) && bytes(sensor_b.getDebugImageDetections()) == rotated(bd);
    const bool black_off = black(bytes(sensor_c.getDebugImageMatches())) && black(bytes(sensor_c.getDebugImageDetections()));
    const bool black_nocb = black(bytes(sensor_d.getDebugImageMatches())) && black(bytes(sensor_d.getDebugImageDetections()));
    const bool black_a = black(bytes(m1)) && black(bytes(d1));
    // with a device: everything holds and each kind was rendered once; without: every picture stays black
    all = all && black_off && black_nocb && (have ? (same_m && same_d && cached && flip_same && after_first - before == 2) : black_a);
    const int err = features_a.lastError() ? features_a.lastError() : static_cast<int>(sensor_a.stats().stats("hip_error"));
    std::printf("frame=%d update=%d hip_error=%d direct=%d matches_same=%d detections_same=%d cached=%d renders=%d flip_same=%d black_off=%d "
                "black_nocb=%d black_a=%d coloured_matches=%d coloured_detections=%d vtx=%d\n",
                k, ok_a ? 1 : 0, ok_a ? 0 : err, have ? 1 : 0, same_m ? 1 : 0, same_d ? 1 : 0, cached ? 1 : 0, after_first - before,
                flip_same ? 1 : 0, black_off ? 1 : 0, black_nocb ? 1 : 0, black_a ? 1 : 0, coloured(bytes(m1)), coloured(bytes(d1)),
                static_cast<int>(sensor_a.stats().stats("num_vtx")));
  }
  if (!all) return 4;
  return ok_a ? 0 : 3;
}
